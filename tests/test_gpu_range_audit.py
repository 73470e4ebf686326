"""Range words of the full-size engines on an MI355X (tests/range_audit.py), and the whole step against float64 autograd
(oracle/torch_ref.py) with Bernoulli targets outside [0, 1].  Tolerances: those of test_gpu_parity.py::test_full_batch_gradients_vs_f64_autograd."""
import os

import numpy as np
import pytest
import torch

from oracle import vae_oracle as vo
from tests.parity_util import relerr
from tests.range_audit import RangeAudit, bern_targets

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def dev():
  assert torch.cuda.is_available()
  return torch.device('cuda:0')


@pytest.fixture(scope='module')
def L():
  from odin_ai_amd import _lib
  return _lib.load()


def _speech():
  from odin_ai_amd.networks import get_networks
  nets = get_networks('speech', n_frames=96, n_mels=80)
  return (nets['encoder'].layers, nets['decoder'].layers, tuple(nets['encoder'].input_shape),
          nets['latents'].event_shape[0])


SPECS = {
    'dsprites': lambda: vo.dsprites_spec(1),
    'shapes3d': lambda: vo.dsprites_spec(3),
    'celeba': lambda: vo.celeba_spec(45, 3),
    'celeba_gauss': lambda: vo.celeba_spec(45, 6),
    'mnist_dense': lambda: vo.mnist_dense_spec(),
    'mnist_conv': lambda: vo.mnist_conv_spec(),
    'speech': _speech,
}

AUDIT_FULL = [
    # the configs of test_gpu_parity.py::FULL (name, spec, B, engine keywords)
    ('dsprites_b256_default', 'dsprites', 256, {}),
    ('dsprites_b256_overlap_small_early_reduce', 'dsprites', 256, dict(overlap_wgrad='small', early_reduce=True)),
    ('dsprites_b256_defer_wgrad', 'dsprites', 256, dict(defer_wgrad=True)),
    ('shapes3d_b128', 'shapes3d', 128, {}),
    ('celeba_b512', 'celeba', 512, {}),
    ('celeba_betatc_b512', 'celeba', 512, dict(tc='betatc')),
    ('mnist_dense_b128', 'mnist_dense', 128, {}),
    ('mnist_conv_b128', 'mnist_conv', 128, {}),
    ('speech_b256', 'speech', 256, dict(observation='gaussian_softplus1')),
    ('dsprites_b256_force_dp', 'dsprites', 256, dict(force_dp=True)),
]


@pytest.mark.parametrize('name,spec,B,kw', AUDIT_FULL, ids=[c[0] for c in AUDIT_FULL])
def test_full_size_range_words(dev, L, name, spec, B, kw):
  """3 eager steps under the audit (beta 1e3 -> 1e-2 -> 1: the gradient scale drops by far more than 10^4), then 3
  graph-replayed steps, each followed by (d): the whole range-word buffer is zero"""
  from odin_ai_amd.engine import VAEEngine
  enc, dec, in_shape, zdim = SPECS[spec]()
  eng = VAEEngine(enc, dec, in_shape, zdim, B, dev, lib=L, **kw)
  g = torch.Generator(device='cpu').manual_seed(1)
  x = torch.rand((B,) + tuple(in_shape), generator=g).clamp_(1e-6, 1 - 1e-6).to(dev)
  audit = RangeAudit(eng)
  for beta in (1e3, 1e-2, 1.0):
    eng.train_step(x, None, lr=1e-3, beta=beta, global_clipnorm=100.0)
    audit.check_cleared()
  assert len(audit.steps) == 3
  if not eng.is_dp:
    audit.check_cover()
  eng.debug_check_ranges = False   # (no host synchronisation inside a capture)
  for beta in (1e3, 1e-2, 1.0):
    eng.train_step(x, None, lr=1e-3, beta=beta, global_clipnorm=100.0, use_graph=True)
    audit.check_cleared()
  assert torch.isfinite(eng.out4).all() and int(eng.flag.item()) == 0
  print(name, 'words checked', audit.n_checked(), 'cover', audit.cover)


def _vs_f64(dev, L, spec, B, x, eps, P, obs='bernoulli', fused=True, audit=True, **ekw):
  """one forward + backward at P against float64 autograd: loss, llk, kl and every gradient within 1e-4"""
  from odin_ai_amd.engine import VAEEngine
  from oracle.torch_ref import TorchVAE
  enc, dec, in_shape, zdim = spec
  kw = dict(beta=1.0, observation=obs)
  torch.set_num_threads(min(16, os.cpu_count() or 1))
  out, G = TorchVAE(enc, dec, in_shape, zdim, **kw).loss_and_grads(P, x.astype(np.float64), eps.astype(np.float64))
  eng = VAEEngine(enc, dec, in_shape, zdim, B, dev, observation=obs, lib=L, **ekw)
  au = RangeAudit(eng, fail_fast=False) if audit else None
  eng.load_params(P)
  eng.step_count = 1
  eng.set_hyper(lr=1e-3, beta=1.0)
  eng.forward(torch.tensor(x, dtype=torch.float32, device=dev), torch.tensor(eps, dtype=torch.float32, device=dev),
              fused=fused)
  eng.backward()
  torch.cuda.synchronize()
  rep = dict(loss=abs(eng.out4[0].item() - float(out['loss'])) / abs(float(out['loss'])),
             llk=relerr(eng.llk.cpu().numpy(), out['llk']),
             kl=relerr(eng.kl.cpu().numpy(), out['kl']))
  gv = {k: v.cpu().numpy() for k, v in eng.grad_views().items()}
  for k in G:
    rep['grad' + str(k)] = relerr(gv[k], G[k])
  worst = max(rep.items(), key=lambda kv: kv[1])
  print('worst relative error', worst)
  assert int(eng.flag.item()) == 0
  for k, v in rep.items():
    assert v <= 1e-4, (k, v)
  if au is not None:
    assert not au.failures, au.failures
  return eng


@pytest.mark.parametrize('spec,B,fused', [('mnist_dense', 128, True), ('dsprites', 32, False), ('dsprites', 32, True)])
def test_bernoulli_targets_outside_unit_interval(dev, L, spec, B, fused):
  """targets in [-2, 6] and exact 0 / 1: the stand-alone ELBO kernel (dense MNIST; the unfused dSprites step) and the
  fused tail keep a valid word for the top gradient -- no NaN flag, loss and gradients as float64"""
  s = SPECS[spec]()
  enc, dec, in_shape, zdim = s
  rng = np.random.default_rng(5)
  eps = rng.standard_normal((B, zdim)).astype(np.float32)
  P = vo.OracleVAE(enc, dec, in_shape, zdim).init_params(seed=9)
  P = {k: v.astype(np.float32).astype(np.float64) for k, v in P.items()}
  _vs_f64(dev, L, s, B, bern_targets((B,) + tuple(in_shape)).astype(np.float32), eps, P, fused=fused)


def test_bernoulli_unit_targets_need_no_absmax(dev, L):
  """targets in [0, 1]: the dense MNIST step runs without a single absmax fallback pass"""
  from odin_ai_amd.engine import VAEEngine
  enc, dec, in_shape, zdim = vo.mnist_dense_spec()
  B = 128
  eng = VAEEngine(enc, dec, in_shape, zdim, B, dev, lib=L)
  x = (torch.rand((B,) + tuple(in_shape), generator=torch.Generator().manual_seed(0)) < 0.13).float().to(dev)
  eng.train_step(x, None, global_clipnorm=100.0)
  torch.cuda.synchronize()
  n0 = L.odin_debug_absmax_fallbacks()
  eng.train_step(x, None, global_clipnorm=100.0)
  torch.cuda.synchronize()
  assert L.odin_debug_absmax_fallbacks() == n0
