"""Range words of a live engine (tests/range_audit.py) on the simulator, and the whole step against float64 with
Bernoulli targets outside [0, 1] (the top gradient's range word).

The audited runs change the gradient scale by far more than 10^4 between consecutive steps (beta 1e3 -> 1e-2): a
word left over from the step before, or the word of another layer, is then looser than the 1.0001 bar."""
import numpy as np
import pytest
import torch

from odin_ai_amd.engine import VAEEngine
from oracle import vae_oracle as vo
from tests.parity_util import check_engine_vs_oracle, make_case
from tests.range_audit import RangeAudit, bern_targets
from tests.simutil import sim_lib
from tests.engine_util import dense_spec, head_spec, neck_spec, tiny16_spec, tiny_spec


@pytest.fixture(scope='module')
def L():
  return sim_lib()


BETAS = (1e3, 1e-2, 1.0)


def audited_steps(eng, x, eps, betas=BETAS, fused=True, clip=100.0):
  """one audited step per beta (forward, backward under the audit, reduction, Adam), (d) after each"""
  audit = RangeAudit(eng)
  tx = torch.as_tensor(np.ascontiguousarray(x), dtype=torch.float32, device=eng.device)
  te = torch.as_tensor(np.ascontiguousarray(eps), dtype=torch.float32, device=eng.device)
  for beta in betas:
    if fused:
      eng.train_step(tx, te, lr=1e-3, beta=beta, global_clipnorm=clip)
    else:
      eng.step_count += 1
      eng.set_hyper(lr=1e-3, beta=beta)
      eng.forward(tx, te, fused=False)
      eng.backward()
      eng.adam(global_clipnorm=clip)
    audit.check_cleared()
    assert torch.isfinite(eng.out4).all() and int(eng.flag.item()) == 0
  assert len(audit.steps) == len(betas) and all(audit.steps)
  return audit


def _spec(name, C=1):
  if name == 'gauss':
    return head_spec(2 * C, 5, C)
  if name == 'mixql':
    return head_spec(10 * vo.mixql_n_out(C), 5, C)
  if name == 'tiny16':
    return tiny16_spec(C)
  if name == 'neck':
    return neck_spec(5, 128, C)
  if name == 'mnist_dense':
    return dense_spec(28)
  return tiny_spec(5, C)


AUDIT_CASES = [
    # (id, spec, observation, engine keywords, fused)
    ('default', 'tiny', 'bernoulli', {}, True),
    ('unfused', 'tiny', 'bernoulli', {}, False),
    ('fused_tail', 'tiny16', 'bernoulli', {}, True),
    ('neck', 'neck', 'bernoulli', {}, True),
    ('betatc', 'tiny', 'bernoulli', dict(tc='betatc'), True),
    ('mmd', 'tiny', 'bernoulli', dict(latent_reg='mmd', reg_coef=5.0), True),
    ('dip_ii', 'tiny', 'bernoulli', dict(latent_reg='dip_ii', reg_coef=2.0), True),
    ('gaussian', 'gauss', 'gaussian_softplus1', {}, True),
    ('qlogistic', 'gauss', 'qlogistic', {}, True),
    ('mixql', 'mixql', 'mixqlogistic', {}, True),
    ('overlap_early', 'tiny', 'bernoulli', dict(overlap_wgrad='small', early_reduce=True), True),
    ('defer_wgrad', 'tiny', 'bernoulli', dict(defer_wgrad=True), True),
    ('mnist_dense', 'mnist_dense', 'bernoulli', {}, True),
]


@pytest.mark.parametrize('cid,spec,obs,kw,fused', AUDIT_CASES, ids=[c[0] for c in AUDIT_CASES])
def test_range_words_of_live_engine(L, cid, spec, obs, kw, fused):
  B = 3
  enc, dec, in_shape, zdim, x, eps = make_case(_spec(spec), obs, B)
  eng = VAEEngine(enc, dec, in_shape, zdim, B, 'cpu', observation=obs, lib=L, **kw)
  if cid == 'neck':
    assert eng.neck
    eng._neck_bwd_opt = True
  if cid == 'default':
    assert eng.lat_block
  g = torch.Generator().manual_seed(5)
  eng.params.copy_(torch.randn(eng.params.numel(), generator=g) * 0.1)
  audit = audited_steps(eng, x, eps, fused=fused)
  if fused:
    audit.check_cover()
  assert audit.n_checked() >= 3 * 3


def test_range_words_model_api_sequence(L):
  """encode -> decode -> optimize: the step after two forward-only passes starts from words the forward passes wrote
  (VAEEngine._clear_stale_act_words): the audit of the optimize step sees no stale activation word"""
  B = 3
  enc, dec, in_shape, zdim, x, eps = make_case(tiny_spec(5), 'bernoulli', B)
  eng = VAEEngine(enc, dec, in_shape, zdim, B, 'cpu', lib=L)
  g = torch.Generator().manual_seed(2)
  eng.params.copy_(torch.randn(eng.params.numel(), generator=g) * 0.1)
  audit = RangeAudit(eng)
  tx = torch.as_tensor(x, dtype=torch.float32)
  te = torch.as_tensor(eps, dtype=torch.float32)
  for scale in (30.0, 1.0):   # (a large batch first: its activation words must not survive into the step)
    eng.set_hyper(beta=1.0)
    eng.run_encoder((tx * scale).contiguous(), te)
    eng.run_decoder((eng.z * scale).contiguous())
    eng.train_step(tx, te, lr=1e-3, beta=1.0, global_clipnorm=100.0)
    audit.check_cleared()
  assert len(audit.steps) == 2


# ---- Bernoulli targets outside [0, 1] ------------------------------------------------------------------------------
@pytest.mark.parametrize('spec,fused', [('mnist_dense', True), ('tiny', False), ('tiny16', True)])
def test_bernoulli_targets_outside_unit_interval(L, spec, fused):
  """the reference's Bernoulli log-prob takes any real target: targets in [-2, 6] (and exact 0 / 1) on the stand-alone
  ELBO kernel (MNIST dense, the unfused conv step) and the fused tail -- no NaN flag, loss and gradients as float64"""
  B = 3
  enc, dec, in_shape, zdim, _, eps = make_case(_spec(spec), 'bernoulli', B)
  x = bern_targets((B,) + tuple(in_shape))
  model = vo.OracleVAE(enc, dec, in_shape, zdim, observation='bernoulli', beta=1.0)
  P = model.init_params(seed=11)
  eng = VAEEngine(enc, dec, in_shape, zdim, B, 'cpu', observation='bernoulli', lib=L)
  if spec == 'tiny16':
    assert eng.fused_tail
  if not fused:
    eng.lat_block = eng.neck = eng.fused_tail = eng.gauss_head = False
  audit = RangeAudit(eng)
  check_engine_vs_oracle(eng, model, P, x, eps, beta=1.0, steps=1, clip=None)
  assert int(eng.flag.item()) == 0
  audit.check_cleared()
