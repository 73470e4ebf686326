"""The continuous Bernoulli observation ('cbernoulli'): the float64 restatement against torch.distributions, the HIP
kernel and head mode 4 against the restatement, whole training steps against float64 autograd, the launch lists, data
parallelism and the model API.  Kernel tolerances: `close` of tests/test_pointwise.py (1e-5 on summed log-likelihoods,
2e-5 on gradients times B, relative to max(1, |ref|max)); step tolerances: the 1e-4 bars of tests/parity_util.py.

The kernel's series / closed-form switch is |l| = 1 (odin_cbern.h); HAND holds the two float32 neighbours on either side."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

from odin_ai_amd import _lib
from odin_ai_amd._lib import OdinError
from odin_ai_amd.engine import VAEEngine
from oracle import vae_oracle as vo
from tests import cbern_util as cb
from tests.engine_util import Recorder, case_data, launch_record, tiny_batch, tiny_nets, tiny_spec
from tests.parity_util import relerr
from tests.test_latent_regularizers import _adam_ref
from tests.test_pointwise import close
from tests.test_vamprior import PLAIN_STEP_CALLS

F64 = torch.float64
SWITCH = np.float32(1.0)
_lo1 = np.nextafter(SWITCH, np.float32(0))
_hi1 = np.nextafter(SWITCH, np.float32(2))
HAND = np.array([0.0, 1e-20, -1e-20, 1e-6, -1e-6, 1e-3, -1e-3,
                 np.nextafter(_lo1, np.float32(0)), _lo1, SWITCH, _hi1,
                 -np.nextafter(_lo1, np.float32(0)), -_lo1, -SWITCH, -_hi1,
                 20.0, -20.0, 88.0, -88.0, 100.0, -100.0, 1e4, -1e4], np.float32)


def sync(bk):
  if bk.dev.type == 'cuda':
    torch.cuda.synchronize()


def f32(a):
  """through float32, as the kernel sees it, back to float64 for the reference"""
  return np.asarray(a, np.float64).astype(np.float32).astype(np.float64)


# ---- 1. the restatement (CPU) -------------------------------------------------------------------------------------------
def test_series_and_closed_forms_agree_where_both_are_accurate():
  a = torch.logspace(-3, -1, 401, dtype=F64)
  l = torch.cat([a, -a])
  assert float((cb.log_norm_series(l) - cb.log_norm_closed(l)).abs().max()) <= 1e-12
  assert float((cb.mean_series(l) - cb.mean_closed(l)).abs().max()) <= 1e-12
  # the two symmetries and the values at 0
  assert float((cb.log_norm(-l) - (cb.log_norm(l) - l)).abs().max()) <= 1e-12
  assert float((cb.mean(-l) - (1 - cb.mean(l))).abs().max()) <= 1e-12
  z = torch.zeros(1, dtype=F64)
  assert float(cb.log_norm(z)) == 0.0 and float(cb.mean(z)) == 0.5


def test_restatement_matches_torch_distributions():
  l = torch.linspace(-12, 12, 4801, dtype=F64)
  keep = ~((torch.sigmoid(l) >= 0.499) & (torch.sigmoid(l) <= 0.501))   # torch's Taylor band around probs = 1/2
  assert float((~keep).sum()) < 0.01 * l.numel()
  l = l[keep].clone().requires_grad_(True)
  x = torch.tensor(np.random.default_rng(0).random(l.numel()), dtype=F64)
  d = torch.distributions.ContinuousBernoulli(logits=l)
  lp_ref = d.log_prob(x)
  g_ref, = torch.autograd.grad(lp_ref.sum(), l)
  lp = cb.log_prob(l, x)
  g, = torch.autograd.grad(lp.sum(), l)
  for got, ref, what in ((lp, lp_ref, 'log_prob'), (g, g_ref, 'gradient'), (cb.mean(l), d.mean, 'mean'),
                         (x - cb.mean(l), g_ref, 'x - mu')):
    err = float((got - ref).detach().abs().max())
    print(f'{what}: {err:.2e}')
    assert err <= 1e-9, (what, err)


@pytest.mark.parametrize('l', [0.0, 1e-12, -1e-12, 1e-3, -1e-3, 0.3, -0.3, 3.0, -3.0, 12.0, -12.0, 30.0, -30.0])
def test_density_is_normalised_and_its_mean_is_mu(l):
  t, w = np.polynomial.legendre.leggauss(96)
  x, w = torch.tensor(0.5 * (t + 1)), torch.tensor(0.5 * w)
  lt = torch.full_like(x, l)
  p = torch.exp(cb.log_prob(lt, x))
  assert abs(float((w * p).sum()) - 1.0) <= 1e-10
  assert abs(float((w * x * p).sum()) - float(cb.mean(lt[:1]))) <= 1e-10


def test_icdf_round_trips_through_the_cdf():
  rng = np.random.default_rng(1)
  l = torch.tensor(np.concatenate([[0.0, 1e-12, -1e-12, 1e-3, -1e-3, 30.0, -30.0], rng.standard_normal(500) * 5]))
  u = torch.tensor(rng.random(l.numel()))
  x = cb.icdf(l, u)
  assert bool(((x >= 0) & (x <= 1)).all())
  assert float((cb.cdf(l, x) - u).abs().max()) <= 1e-12
  assert torch.equal(cb.icdf(torch.zeros(3, dtype=F64), u[:3]), u[:3])


# ---- 2. the kernel against the restatement ------------------------------------------------------------------------------
def kernel_inputs(B, n, seed=1):
  """logits 3 N(0, 1); targets uniform in [1e-6, 1 - 1e-6] with an exact 0 and an exact 1 where there is room; where a row
  holds them, HAND opens row 0"""
  rng = np.random.default_rng(seed)
  lg = f32(rng.standard_normal((B, n)) * 3)
  x = f32(np.clip(rng.random((B, n)), 1e-6, 1 - 1e-6))
  if n >= HAND.size:
    lg[0, :HAND.size] = HAND
  if n >= 2:
    x[0, 0], x[-1, -1] = 0.0, 1.0
  return lg, x


def run_kernel(bk, lg, x, x_offset=0, word=True):
  """-> (parts [B, n_part], dlogits [B, n], the range word or None); x_offset: floats the target pointer is shifted by"""
  L, T = bk.L, bk.T
  B, n = lg.shape
  npart, dry = C.c_int(0), C.c_int(0)
  L.odin_elbo_cbernoulli_fwd_bwd(None, None, None, None, None, B, n, C.byref(dry), None, None)
  tl, sc = T(lg), T([1.0 / B])
  xbuf = bk.zeros(B * n + 4)
  tx = xbuf[x_offset:x_offset + B * n]
  tx.copy_(T(x).reshape(-1))
  assert tx.data_ptr() % 16 == (4 * x_offset) % 16
  part, dl = bk.full((B * dry.value,), float('nan')), bk.full((B, n), float('nan'))
  w = bk.zeros(2048, dtype=torch.int32) if word else None
  L.odin_elbo_cbernoulli_fwd_bwd(tl.data_ptr(), tx.data_ptr(), part.data_ptr(), dl.data_ptr(), sc.data_ptr(), B, n,
                                 C.byref(npart), None if w is None else w.data_ptr(), None)
  sync(bk)
  assert npart.value == dry.value >= 1   # the dry run reports what the real run uses
  return part.reshape(B, -1), dl, w


def check_kernel(bk, B, n, x_offset=0):
  lg, x = kernel_inputs(B, n)
  part, dl, w = run_kernel(bk, lg, x, x_offset)
  l64, x64 = cb.t64(lg), cb.t64(x)
  llk_ref = cb.log_prob_sum(l64, x64).numpy()
  dl_ref = -(x64 - cb.mean(l64)).numpy() / B
  got = part.cpu().numpy().astype(np.float64)
  assert np.isfinite(got).all() and bool(torch.isfinite(dl).all())
  close(got.sum(1), llk_ref, 1e-5)
  close(dl.cpu().numpy() * B, dl_ref * B)
  amax = float(w.view(torch.float32).max())
  assert amax == float(dl.abs().max()) and amax <= 1.0 / B
  return part, dl, llk_ref


# (1, 1) | not a multiple of 4: the scalar path | one element group past a chunk edge | the vector path
@pytest.mark.parametrize('B,n', [(1, 1), (3, 21), (2, 1028), (3, 4096)])
def test_kernel_matches_float64(bk, B, n):
  check_kernel(bk, B, n)


def test_kernel_with_an_unaligned_target_pointer(bk):
  part, dl, _ = check_kernel(bk, 3, 4096, x_offset=1)
  part2, dl2, _ = check_kernel(bk, 3, 4096)
  # the same elements in the same chunks: only the access width differs
  assert part.shape == part2.shape and torch.equal(dl, dl2)


@pytest.mark.parametrize('x_offset', [0, 1])
def test_kernel_grid_stride_form(bk, x_offset):
  """(256, 4096) = 2^20 elements with n_per % 256 == 0: the smallest shape the launcher sends to the persistent kernel
  (aligned) / to one wave per 256-element chunk (unaligned): n_per / 256 partials per sample either way"""
  if bk.name == 'sim':
    pytest.skip('large shapes run on the GPU backend only (fiber simulator: minutes)')
  part, dl, _ = check_kernel(bk, 256, 4096, x_offset)
  assert part.shape == (256, 16)
  part2, dl2, _ = check_kernel(bk, 256, 4096, x_offset)   # a second launch: equal bits
  assert torch.equal(part, part2) and torch.equal(dl, dl2)


def test_kernel_hand_placed_logits_one_by_one(bk):
  """every hand-placed logit against targets 0, 0.3 and 1 as a sample of its own (n_per = 1): the log-likelihood of each
  element is visible, and is held to 1e-5 of max(1, |its own reference|)"""
  lg = f32(np.repeat(HAND, 3))[:, None]
  x = f32(np.tile([0.0, 0.3, 1.0], HAND.size))[:, None]
  B = lg.shape[0]
  part, dl, w = run_kernel(bk, lg, x)
  assert part.shape == (B, 1)
  got, g = part.cpu().numpy().astype(np.float64)[:, 0], dl.cpu().numpy().astype(np.float64)[:, 0] * B
  ref = cb.np_log_prob_sum(lg, x)
  gref = -(x[:, 0] - cb.np_mean(lg[:, 0]))
  assert np.isfinite(got).all() and np.isfinite(g).all()
  err = np.abs(got - ref) / np.maximum(1.0, np.abs(ref))
  assert err.max() <= 1e-5, (float(err.max()), float(lg[err.argmax(), 0]))
  assert np.abs(g - gref).max() <= 2e-5, float(lg[np.abs(g - gref).argmax(), 0])
  # l = 0: llk = 0 and dlogits = -(x - 1/2) / B to rounding
  z = lg[:, 0] == 0
  assert z.sum() == 3 and (got[z] == 0).all()
  want = (-(x[z, 0].astype(np.float32) - np.float32(0.5)) * np.float32(1.0 / B)).astype(np.float32)
  assert np.array_equal(dl.cpu().numpy()[z, 0], want)
  assert float(w.view(torch.float32).max()) <= 1.0 / B


def test_kernel_partials_feed_elbo_finalize(bk):
  L, T = bk.L, bk.T
  B, n = 3, 4096
  lg, x = kernel_inputs(B, n)
  part, _, _ = run_kernel(bk, lg, x)
  llk_ref = cb.np_log_prob_sum(lg, x)
  kl = np.random.default_rng(2).random(B) * 5
  tkl, hyper, ttc = T(kl), T([4.0, 0.5]), T([0.5])
  llk, out = bk.zeros(B), bk.zeros(4)
  L.odin_elbo_finalize(part.data_ptr(), part.shape[1], tkl.data_ptr(), hyper.data_ptr(), ttc.data_ptr(), llk.data_ptr(),
                       out.data_ptr(), B, None)
  close(llk.cpu().numpy(), llk_ref, 1e-5)
  loss = -(llk_ref.mean() - 4.0 * kl.mean() - 0.25)
  close(out.cpu().numpy(), [loss, llk_ref.mean(), 4.0 * kl.mean(), 0.25], 1e-5)


def test_kernel_refuses_bad_sizes_and_touches_nothing(bk):
  L = bk.L
  tl, tx, sc = bk.zeros(8), bk.zeros(8), bk.full((1,), 0.5)
  part, dl, w = bk.full((8,), 7.0), bk.full((8,), 7.0), bk.zeros(2048, dtype=torch.int32)
  npart = C.c_int(-5)
  for B, n in ((0, 8), (-1, 8), (2, 0), (2, -4)):
    with pytest.raises(OdinError, match='rc=-2'):
      L.odin_elbo_cbernoulli_fwd_bwd(tl.data_ptr(), tx.data_ptr(), part.data_ptr(), dl.data_ptr(), sc.data_ptr(), B, n,
                                     C.byref(npart), w.data_ptr(), None)
  sync(bk)
  assert npart.value == -5 and bool((part == 7.0).all()) and bool((dl == 7.0).all()) and bool((w == 0).all())


# the scalar path | the vector path past a chunk edge | the vector path | the scalar path of an unaligned pointer
# (the two forms of >= 2^20 elements are launched twice in test_kernel_grid_stride_form)
@pytest.mark.parametrize('B,n,x_offset', [(3, 21, 0), (2, 1028, 0), (3, 4096, 0), (3, 4096, 1)])
def test_kernel_is_bit_reproducible(bk, B, n, x_offset):
  lg, x = kernel_inputs(B, n)
  a, b = run_kernel(bk, lg, x, x_offset), run_kernel(bk, lg, x, x_offset)
  assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and torch.equal(a[2], b[2])


# ---- 3. head mode 4 -----------------------------------------------------------------------------------------------------
HEAD_CASES = [(3, 300, 32, 1, 'elu', False), (2, 784, 32, 1, 'relu', False), (2, 530, 16, 3, 'elu', False),
              (2, 300, 32, 1, 'elu', True)]   # (the last: zero weights and a tiny bias, logits within 1e-3 of 0)


@pytest.mark.parametrize('B,npix,Cin,Cc,hact,flat', HEAD_CASES)
def test_cbernoulli_head(bk, B, npix, Cin, Cc, hact, flat):
  """odin_gaussian_head_fwd_bwd with softplus1 = 4: Conv2D 1x1 -> ContinuousBernoulli(logits) log-prob -> backward"""
  L, T = bk.L, bk.T
  rng = np.random.default_rng(14)
  pre = rng.standard_normal((B, npix, Cin))
  h = f32({'elu': vo.elu, 'relu': lambda a: np.maximum(a, 0.0)}[hact](pre))
  w1 = np.zeros((Cin, Cc)) if flat else f32(rng.standard_normal((Cin, Cc)) * 0.3)
  b1 = f32([7e-4, -3e-4, 0.0][:Cc]) if flat else f32(rng.standard_normal(Cc) * 0.1)
  x = f32(np.clip(rng.random((B, npix, Cc)), 1e-6, 1 - 1e-6))
  lg = h @ w1 + b1
  assert not flat or np.abs(lg).max() <= 1e-3
  l64, x64 = cb.t64(lg), cb.t64(x)
  llk_ref = cb.log_prob_sum(l64, x64).numpy()
  dl_ref = -(x64 - cb.mean(l64)).numpy() / B
  hgrad = {'relu': (h > 0).astype(np.float64), 'elu': vo.elu_grad_from_output(h)}[hact]
  dh_ref = (dl_ref @ w1.T) * hgrad
  th, tw, tb, tx, sc = T(h), T(w1), T(b1), T(x), T([1.0 / B])
  npart, rows = C.c_int(0), C.c_int(0)
  L.odin_gaussian_head_fwd_bwd(None, None, None, None, None, None, None, None, C.byref(npart), None, C.byref(rows),
                               None, None, B, npix, Cin, Cc, 4, 0, None, None)
  logits, dl, dh = bk.zeros(B, npix, Cc), bk.zeros(B, npix, Cc), bk.full((B, npix, Cin), float('nan'))
  part = bk.full((B * npart.value,), float('nan'))
  slab = bk.full((rows.value, Cin * Cc + Cc), float('nan'))
  cs = bk.full((rows.value, Cin), float('nan'))
  word = bk.zeros(2048, dtype=torch.int32)
  L.odin_gaussian_head_fwd_bwd(th.data_ptr(), tw.data_ptr(), tb.data_ptr(), tx.data_ptr(), logits.data_ptr(),
                               dl.data_ptr(), dh.data_ptr(), part.data_ptr(), C.byref(npart), slab.data_ptr(),
                               C.byref(rows), cs.data_ptr(), sc.data_ptr(), B, npix, Cin, Cc, 4, _lib.ACT[hact],
                               word.data_ptr(), None)
  sync(bk)
  close(logits.cpu().numpy(), lg)
  close(part.reshape(B, -1).sum(1).cpu().numpy(), llk_ref, 1e-5)
  close(dl.cpu().numpy() * B, dl_ref * B)
  close(dh.cpu().numpy() * B, dh_ref * B)
  g = slab.cpu().numpy().astype(np.float64).sum(0)
  close(g[:Cin * Cc].reshape(Cin, Cc), np.einsum('bpc,bpo->co', h, dl_ref), 1e-4)
  close(g[Cin * Cc:], dl_ref.sum((0, 1)), 1e-4)
  close(cs.cpu().numpy().astype(np.float64).sum(0), dh_ref.sum((0, 1)), 1e-4)
  assert float(word.view(torch.float32).max()) == float(dh.abs().max())


# ---- 4. whole training steps against float64 autograd -------------------------------------------------------------------
def dsprites_tail_spec(zdim=4):
  """8 x 8 x 1 with the dSprites decoder's tail: Conv2DTranspose(32 -> 32, k4, s2) -> Conv2D 1x1 (the head sees Cin = 32)"""
  enc, _, shp, _ = tiny_spec(zdim)
  dec = [('dense', 128, 'linear'), ('reshape', (2, 2, 32)), ('deconv', 32, 4, 2, 'elu'), ('deconv', 32, 4, 2, 'elu'),
         ('conv', 1, 1, 1, 'linear')]
  return enc, dec, shp, zdim


def step_case(bk, spec, B, calls=None, **kw):
  enc, dec, in_shape, D = spec
  lib = bk.L if calls is None else Recorder(bk.L, calls)
  eng = VAEEngine(enc, dec, in_shape, D, B, bk.dev, lib=lib, observation='cbernoulli', **kw)
  P = vo.OracleVAE(enc, dec, in_shape, D, observation='bernoulli').init_params(seed=5)
  P = {k: f32(v) for k, v in P.items()}
  eng.load_params(P)
  rng = np.random.default_rng(7)
  x = np.clip(rng.random((B,) + tuple(in_shape)), 1e-6, 1 - 1e-6).astype(np.float32)
  return eng, P, x, rng.standard_normal((B, D)).astype(np.float32)


STEP_CASES = [('c1_b4', lambda: tiny_spec(4, 1), 4), ('c3_b6', lambda: tiny_spec(4, 3), 6),
              ('dsprites_tail_b2', dsprites_tail_spec, 2)]


@pytest.mark.parametrize('fused', [True, False], ids=['head', 'unfused'])
@pytest.mark.parametrize('cid,spec,B', STEP_CASES, ids=[c[0] for c in STEP_CASES])
def test_three_steps_follow_float64_autograd(bk, cid, spec, B, fused):
  spec, lr, beta, tol = spec(), 1e-3, 2.0, 1e-4
  calls = []
  eng, P, x, eps = step_case(bk, spec, B, calls)
  assert eng.gauss_head and eng.head_mode == 4 and not eng.fused_tail and not eng.chain_tail
  ref = cb.CBernRef(spec[0], spec[1], spec[3], beta)
  M = {k: np.zeros_like(v) for k, v in P.items()}
  V = {k: np.zeros_like(v) for k, v in P.items()}
  xt, et = bk.T(x), bk.T(eps)
  for t in (1, 2, 3):
    f, G = ref.loss_and_grads(P, x, eps)
    eng.step_count = t
    eng.set_hyper(lr=lr, beta=beta)
    calls.clear()
    eng.forward(xt, et, fused=fused)
    eng.backward()
    sync(bk)
    # the launch list: layer[-2] | head, or layer[-2] | 1x1 conv | the stand-alone kernel
    elbo = [c for c in calls if c.startswith('odin_elbo_') and c != 'odin_elbo_finalize']
    assert calls.count('odin_gaussian_head_fwd_bwd') == (1 if fused else 0)
    assert elbo == ([] if fused else ['odin_elbo_cbernoulli_fwd_bwd'])
    assert not [c for c in calls if c.startswith('odin_bernoulli_tail_') or c == 'odin_decoder_tail_chain']
    rep = dict(h_d=relerr(eng.dec.outs[-1].cpu().numpy().reshape(f['h_d'].shape), f['h_d']),
               llk=relerr(eng.llk.cpu().numpy(), f['llk']),
               kl=np.abs(eng.kl.cpu().numpy() - f['kl']).max() / max(1.0, np.abs(f['kl']).max()),
               loss=abs(float(eng.out4[0]) - f['loss']) / max(1.0, abs(f['loss'])))
    gv = {k: v.cpu().numpy() for k, v in eng.grad_views().items()}
    assert set(gv) == set(G)
    for k in G:
      rep['grad' + str(k)] = relerr(gv[k], G[k])
    for k, v in rep.items():
      assert v <= tol, (t, k, v)
    eng.adam()
    _adam_ref(P, G, M, V, t, lr)
    pv = {k: v.cpu().numpy() for k, v in eng.param_views().items()}
    for k in P:
      # (parity_util's bars: 1e-4 where the gradient is well conditioned, the mean error below 0.5 % of the step size)
      d = np.abs(pv[k] - P[k])
      good = np.abs(G[k]) > 1e-3 * np.abs(G[k]).max()
      assert d[good].max() <= tol, (t, 'param', k, float(d[good].max()))
      assert d.mean() <= 5e-3 * lr, (t, 'param-mean', k, float(d.mean()))
    eng.load_params(P)   # continue from the reference's parameters: errors do not compound in the check


def test_train_step_call_list(bk):
  calls = []
  eng, P, x, eps = step_case(bk, tiny_spec(), 4, calls)
  calls.clear()
  out = eng.train_step(bk.T(x), bk.T(eps), lr=1e-3, beta=2.0)
  sync(bk)
  assert bool(torch.isfinite(out).all())
  assert calls.count('odin_gaussian_head_fwd_bwd') == 1
  assert not [c for c in calls if (c.startswith('odin_elbo_') and c != 'odin_elbo_finalize')
              or c.startswith('odin_bernoulli_tail_') or c == 'odin_decoder_tail_chain']
  # a decoder without a 1x1 head: the stand-alone kernel, which keeps the top gradient's range word itself
  from tests.engine_util import dense_spec
  calls2 = []
  eng2 = VAEEngine(*dense_spec(), 4, bk.dev, lib=Recorder(bk.L, calls2), observation='cbernoulli')
  x2, eps2 = case_data(bk.dev, dense_spec())
  calls2.clear()
  eng2.train_step(x2, eps2, lr=1e-3, beta=2.0)
  sync(bk)
  assert not eng2.gauss_head and eng2._bern_keeps_top and calls2.count('odin_elbo_cbernoulli_fwd_bwd') == 1
  assert 'odin_absmax' not in calls2 and bool(torch.isfinite(eng2.out4).all())


@pytest.mark.gpu
def test_graph_replay_equals_eager_and_sees_the_beta_schedule():
  from tests.test_latent_regularizers import _Hip
  bk = _Hip()
  res = []
  for use_graph in (False, True):
    eng, P, x, eps = step_case(bk, tiny_spec(), 4)
    xt, et = bk.T(x), bk.T(eps)
    outs = [eng.train_step(xt, et, lr=1e-3, beta=b, use_graph=use_graph).clone() for b in (0.5, 1.0, 2.0, 4.0)]
    sync(bk)
    res.append([eng.params.clone(), torch.stack(outs), eng.dp.clone(), eng.llk.clone()])
  for a, b in zip(res[0], res[1]):
    assert torch.equal(a, b)
  assert bool(torch.isfinite(res[0][1]).all()) and len(set(res[0][1][:, 2].tolist())) == 4
  # a beta change between two replays is seen: the KL term scales, the likelihood does not
  eng, P, x, eps = step_case(bk, tiny_spec(), 4)
  xt, et = bk.T(x), bk.T(eps)
  o1 = eng.train_step(xt, et, lr=0.0, beta=1.0, use_graph=True).clone()
  o2 = eng.train_step(xt, et, lr=0.0, beta=3.0, use_graph=True).clone()
  assert float(o1[1]) == float(o2[1]) and abs(float(o2[2]) - 3.0 * float(o1[2])) <= 1e-5 * abs(float(o2[2]))


# ---- 5. existing paths unchanged ----------------------------------------------------------------------------------------
def test_plain_bernoulli_call_list_is_unchanged(bk):
  eng, c1 = launch_record(bk)
  assert c1 == PLAIN_STEP_CALLS and eng.observation == 'bernoulli'
  assert 'odin_elbo_cbernoulli_fwd_bwd' not in c1


# ---- 6. data parallel ---------------------------------------------------------------------------------------------------
def test_data_parallel_two_ranks(bk):
  from tests.test_dp_one_device import check, run_sharded, run_single
  engs, outs, kinds = run_sharded(bk, 2, 4.0, dp_buckets=2, observation='cbernoulli')
  assert kinds == 'kckck' and all(e.observation == 'cbernoulli' and e.B == 4 for e in engs)
  eng1, outs1 = run_single(bk, 4.0, observation='cbernoulli')
  check(engs, eng1, outs, outs1, term=False)


# ---- 7. the model API ---------------------------------------------------------------------------------------------------
def cb_nets(C=1, zdim=4, latents=None, **obs_kwargs):
  from odin_ai_amd.networks import RVconf
  nets = tiny_nets(C=C, zdim=zdim)
  nets['observation'] = RVconf((8, 8, C), 'cbernoulli', projection=False, name='image', kwargs=dict(obs_kwargs))
  if latents is not None:
    nets['latents'] = latents
  return nets


@pytest.mark.parametrize('name,C', [('mnist', 1), ('dsprites', 1), ('shapes3d', 3), ('celeba', 3), ('dense', 1)])
def test_get_networks_takes_the_distribution(name, C):
  from odin_ai_amd.networks import get_networks
  nets = get_networks(name, distribution='cbernoulli')
  assert nets['observation'].posterior == 'cbernoulli' and nets['observation'].event_shape[-1] == C
  last = [l for l in nets['decoder'].layers if l[0] in ('conv', 'dense')][-1]
  bern = [l for l in get_networks(name)['decoder'].layers if l[0] in ('conv', 'dense')][-1]
  assert last == bern and (last[1] == C if last[0] == 'conv' else last[1] == 28 * 28)
  with pytest.raises(ValueError, match='cbernoulli'):
    get_networks(name, distribution='poisson')


def test_api_fit_call_and_the_observation(bk):
  from odin_ai_amd.vae import BetaVAE, ContinuousBernoulliObservation
  vae = BetaVAE(beta=2.0, device=bk.dev, lib=bk.L, **cb_nets())
  x, eps = tiny_batch(2, B=8)
  vae.fit(x, max_iter=3, batch_size=8, learning_rate=1e-3, compile_graph=False)
  assert vae.step == 3 and np.isfinite(float(vae.optimize(x, training=False)[0]))
  px, qz = vae(x, eps=eps)
  assert isinstance(px, ContinuousBernoulliObservation)
  assert px.event_shape == (8, 8, 1) and px.batch_shape == (8,) and px.logits.shape == (8, 8, 8, 1)
  l64, x64 = cb.t64(px.logits.cpu().numpy()), cb.t64(x)
  close(px.mean().cpu().numpy(), cb.mean(l64).numpy())
  close(px.probs.cpu().numpy(), torch.sigmoid(l64).numpy())
  lp = px.log_prob(torch.as_tensor(x, device=px.logits.device))
  close(lp.cpu().numpy(), cb.log_prob_sum(l64, x64).numpy(), 1e-5)
  llk, kl = vae.elbo_components(x, eps=eps)
  assert llk['llk_image'].shape == (8,) and kl['kl_latents'].shape == (8,)
  close(llk['llk_image'].cpu().numpy(), lp.cpu().numpy(), 1e-5)
  close(llk['llk_image'].cpu().numpy(), cb.log_prob_sum(l64, x64).numpy(), 1e-5)
  assert np.isfinite(vae.elbo(llk, kl).cpu().numpy()).all()
  s = px.sample(3)
  assert s.shape == (3, 8, 8, 8, 1) and bool(((s >= 0) & (s <= 1)).all()) and px.sample().shape == (8, 8, 8, 1)
  # logits exactly 0: the mean is exactly 1/2, nothing divides 0 by 0; tiny and huge logits stay finite and inside [0, 1]
  edge = ContinuousBernoulliObservation(torch.tensor([[0.0, 1e-20, -1e-6, 1e-3, 0.999, -1.0, 30.0, -1e4]], device=bk.dev))
  m = edge.mean()
  assert float(m[0, 0]) == 0.5 and bool(torch.isfinite(m).all()) and bool(((m > 0) & (m < 1)).all())
  close(m.cpu().numpy(), cb.mean(cb.t64(edge.logits.cpu().numpy())).numpy())
  assert bool(torch.isfinite(edge.log_prob(torch.full((1, 8), 0.3, device=bk.dev))).all())
  # saturated logits: x l and max(l, 0) cancel; each element to 1e-5 of max(1, |its own reference|), as in the kernel
  sl = np.array([[1e4], [1e4], [-1e4], [100.0], [88.0], [-20.0]], np.float32)
  sx = np.array([[1.0], [0.3], [0.0], [1.0], [1.0], [1.0]], np.float32)
  got = ContinuousBernoulliObservation(torch.tensor(sl, device=bk.dev)).log_prob(torch.tensor(sx, device=bk.dev))
  want = cb.np_log_prob_sum(sl, sx)
  assert (np.abs(got.cpu().numpy() - want) / np.maximum(1.0, np.abs(want))).max() <= 1e-5
  es = edge.sample(5)
  assert bool(torch.isfinite(es).all()) and bool(((es >= 0) & (es <= 1)).all())
  # the sampler is the inverse CDF: the sample mean over many draws approaches mu
  many = ContinuousBernoulliObservation(torch.tensor([[2.5, -0.7]], device=bk.dev)).sample(20000).mean(0)
  assert np.abs(many.cpu().numpy() - cb.np_mean(np.array([[2.5, -0.7]]))).max() <= 0.01
  ps = vae.sample_observation(2)
  assert isinstance(ps, ContinuousBernoulliObservation) and ps.logits.shape == (2, 8, 8, 1)
  assert isinstance(vae.decode(vae.encode(x, eps=eps)), ContinuousBernoulliObservation)
  assert vae.variable_name(('lat', 'w')) == 'latents/kernel'


def test_marginal_log_prob_matches_float64_logmeanexp(bk):
  from odin_ai_amd.vae import VariationalAutoencoder
  from oracle.torch_ref import TorchVAE, t_seq
  D, n, N = 4, 3, 6
  vae = VariationalAutoencoder(device=bk.dev, lib=bk.L, **cb_nets())
  x, _ = tiny_batch(3, B=N)
  eps = np.random.default_rng(4).standard_normal((n, N, D)).astype(np.float32)
  llk, lat = vae.marginal_log_prob(x, n_mcmc=n, reduce=None, batch_size=4, eps=eps)
  T = {k: torch.as_tensor(v.cpu().numpy(), dtype=F64) for k, v in vae.trainable_variables.items()}
  x64 = torch.as_tensor(x, dtype=F64)
  h_e = t_seq(vae.encoder.layers, TorchVAE._sub(T, 'enc'), x64)
  p = h_e @ T[('lat', 'w')] + T[('lat', 'b')]
  z = p[None, :, :D] + torch.nn.functional.softplus(p[None, :, D:]) * cb.t64(eps)
  h_d = t_seq(vae.decoder.layers, TorchVAE._sub(T, 'dec'), z.reshape(n * N, D)).reshape((n, N, 8, 8, 1))
  lp = cb.log_prob(h_d, x64[None].expand_as(h_d)).reshape(n, N, -1).sum(-1)
  want = (torch.logsumexp(lp, 0) - math.log(n)).numpy()
  got = llk['image'].cpu().numpy()
  assert np.abs(got - want).max() <= 1e-4 * max(1.0, np.abs(want).max())


@pytest.mark.parametrize('fmt', ['npz', 'tf'])
def test_api_save_load_round_trip(bk, tmp_path, fmt):
  from odin_ai_amd.vae import BetaVAE
  vae = BetaVAE(beta=2.0, device=bk.dev, lib=bk.L, **cb_nets())
  x, eps = tiny_batch(2)
  vae.optimize(x, learning_rate=1e-2)
  path = str(tmp_path / 'w')
  vae.save_weights(path, save_format=fmt)
  plain = BetaVAE(beta=2.0, device=bk.dev, lib=bk.L, **tiny_nets())
  # variable names and shapes are the Bernoulli model's
  assert {vae.variable_name(k): tuple(v.shape) for k, v in vae.trainable_variables.items()} == \
         {plain.variable_name(k): tuple(v.shape) for k, v in plain.trainable_variables.items()}
  other = BetaVAE(beta=2.0, device=bk.dev, lib=bk.L, seed=3, **cb_nets())
  assert not torch.equal(other.trainable_variables[('lat', 'w')], vae.trainable_variables[('lat', 'w')])
  other.load_weights(path, raise_notfound=True)
  assert other.step == 1
  for k, v in vae.trainable_variables.items():
    assert torch.equal(v, other.trainable_variables[k]), k
  a, b = vae.elbo_components(x, eps=eps), other.elbo_components(x, eps=eps)
  assert torch.equal(a[0]['llk_image'], b[0]['llk_image']) and torch.equal(a[1]['kl_latents'], b[1]['kl_latents'])


@pytest.mark.parametrize('name', ['vae', 'betavae', 'annealingvae', 'betatcvae', 'factorvae', 'betacapacityvae', 'infovae',
                                  'dipvae', 'vampriorvae', 'vqvae'])
def test_every_model_class_takes_the_observation(bk, name):
  from odin_ai_amd.vae import get_vae
  x, _ = tiny_batch(2, B=8)
  kw = dict(discriminator_units=(16, 16)) if name == 'factorvae' else {}
  vae = get_vae(name)(device=bk.dev, lib=bk.L, **kw, **cb_nets())
  vae.fit(x, max_iter=2, batch_size=8, learning_rate=1e-3, compile_graph=False)   # (factorvae: 4 + 4 of the 8)
  assert vae.step == 2
  assert all(eng.observation == 'cbernoulli' for eng in vae._engines.values())
  loss, _ = vae.optimize(x, training=False)
  assert np.isfinite(float(loss))
  llk, kl = vae.elbo_components(x[:4] if name == 'factorvae' else x)
  assert bool(torch.isfinite(llk['llk_image']).all())
  assert all(bool(torch.isfinite(torch.as_tensor(v)).all()) for v in kl.values())


@pytest.mark.parametrize('alias', ['relaxedonehot', 'mvntril'])
def test_other_posteriors_take_the_observation(bk, alias):
  from odin_ai_amd.networks import RVconf
  from odin_ai_amd.vae import BetaVAE, ContinuousBernoulliObservation
  vae = BetaVAE(beta=2.0, device=bk.dev, lib=bk.L,
                **cb_nets(zdim=5, latents=RVconf(5, alias, projection=True, name='latents')))
  x, _ = tiny_batch(2)
  vae.fit(x, max_iter=2, batch_size=6, learning_rate=1e-3, compile_graph=False)
  llk, kl = vae.elbo_components(x)
  px, _ = vae.last_outputs
  assert isinstance(px, ContinuousBernoulliObservation) and vae._engine(6).observation == 'cbernoulli'
  assert bool(torch.isfinite(llk['llk_image']).all()) and bool(torch.isfinite(kl['kl_latents']).all())
  close(llk['llk_image'].cpu().numpy(), cb.np_log_prob_sum(px.logits.cpu().numpy(), x), 1e-5)


def test_lims_is_accepted_and_ignored(bk):
  from odin_ai_amd.vae import VariationalAutoencoder
  x, eps = tiny_batch(2)
  res = []
  for kw in ({}, dict(lims=(0.4, 0.6))):
    vae = VariationalAutoencoder(device=bk.dev, lib=bk.L, **cb_nets(**kw))
    loss, _ = vae.optimize(x, learning_rate=1e-3, eps=eps)
    llk, kl = vae.elbo_components(x, eps=eps)
    res.append([torch.as_tensor(loss).clone(), vae._params.clone(), llk['llk_image'].clone(), kl['kl_latents'].clone()])
  for a, b in zip(*res):
    assert torch.equal(a, b)
