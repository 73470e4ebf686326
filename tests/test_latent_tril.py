"""The full-covariance Gaussian posterior 'mvntril' (latent_tril.hip, VAEEngine(latent_cov='tril'), MVNTriLPosterior) on
both backends of the `bk` fixture: the fill map, the float64 restatement of tests/tril_util.py against torch's own
MultivariateNormal and autograd, the three kernels against that restatement, whole training steps against float64
autograd, the engine's behaviour and the model API.

Tolerances: 1e-4 of a tensor's maximum for values and gradients (the project's parity bound); the restatement against
torch.distributions to 1e-9; fbmask and everything the kernels promise bit for bit, exactly.

Free bits "clamp some but not all samples": the threshold (and the capacity) lies in the middle of the (second)
widest gap between two KL values of the drawn batch (asserted: both kinds occur, and no sample sits within twice the
parity bound of a threshold).  A batch of ONE sample cannot hold both kinds: there the kernel runs once under a threshold
above the sample's KL and once under one below it.

Whole steps: the loss and the projection's gradient at the parity bound; every element of every parameter after three
Adam steps to 2e-4 of its tensor's largest weight, the bar of the other models' step tests (tests/test_vq.py)."""
import math

import numpy as np
import pytest
import torch

from odin_ai_amd._lib import OdinError
from odin_ai_amd.engine import RANGE_WORDS, VAEEngine
from oracle import vae_oracle as vo
from tests import tril_util as tu
from tests.engine_util import Recorder, case_data, launch_record, neck_spec, tiny_nets, tiny_spec
from tests.range_audit import RangeAudit
from tests.test_latent_regularizers import _adam_ref
from tests.test_vamprior import PLAIN_STEP_CALLS

I32 = torch.int32
F64 = torch.float64


def close(got, ref, tol=1e-4):
  got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
  scale = max(float(np.abs(ref).max()), 1e-30)
  err = float(np.abs(got - ref).max())
  assert err <= tol * scale, (err, scale)


def sync(bk):
  if bk.dev.type == 'cuda':
    torch.cuda.synchronize()


# ---- 1. the fill map ----------------------------------------------------------------------------------------------------
def test_fill_known_answer():
  L = tu.fill_triangular(torch.arange(1.0, 7.0, dtype=F64), 3)
  assert L.tolist() == [[4, 0, 0], [6, 5, 0], [3, 2, 1]]
  for i in range(3):
    for j in range(i + 1):
      assert tu.fill_index(i, j, 3) + 1 == L[i, j]
  from odin_ai_amd.vae import fill_scale_tril
  P = fill_scale_tril(torch.arange(1.0, 7.0, dtype=F64), 3)
  assert torch.equal(torch.tril(P, -1), torch.tril(L, -1))
  assert torch.allclose(torch.diagonal(P), tu.softplus(torch.diagonal(L)) + 1e-5, rtol=0, atol=1e-12)


def test_fill_index_is_a_bijection_for_every_d():
  for D in range(1, 65):
    M = tu.n_tril(D)
    idx = [tu.fill_index(i, j, D) for i in range(D) for j in range(i + 1)]
    assert sorted(idx) == list(range(M)), D
    # and it is the documented construction: r = 0 .. M-1 lands where the formula says
    L = tu.fill_triangular(torch.arange(M, dtype=F64), D)
    got = [int(L[i, j]) for i in range(D) for j in range(i + 1)]
    assert got == idx, D


# ---- 2. the restatement against torch's own distribution ----------------------------------------------------------------
def _draw64(B, D, seed):
  g = torch.Generator().manual_seed(seed)
  p = torch.randn(B, D + tu.n_tril(D), generator=g, dtype=F64) * 0.6
  return p, torch.randn(B, D, generator=g, dtype=F64)


@pytest.mark.parametrize('D', [1, 2, 5, 12])
def test_restatement_matches_torch_multivariate_normal(D):
  from torch.distributions import MultivariateNormal, kl_divergence
  p, eps = _draw64(6, D, 10 + D)
  loc, _, L = tu.split(p, D)
  q = MultivariateNormal(loc, scale_tril=L)
  prior = MultivariateNormal(torch.zeros(D, dtype=F64), scale_tril=torch.eye(D, dtype=F64))
  z = tu.sample(loc, L, eps)
  tol = dict(rtol=0, atol=1e-9)
  assert torch.allclose(tu.log_q(L, eps), q.log_prob(z), **tol)
  assert torch.allclose(tu.log_p(z), prior.log_prob(z), **tol)
  assert torch.allclose(tu.kl_closed(loc, L), kl_divergence(q, prior), **tol)
  assert torch.allclose(tu.kl_mc(loc, L, eps), q.log_prob(z) - prior.log_prob(z), **tol)


@pytest.mark.parametrize('analytic', [False, True])
@pytest.mark.parametrize('D', [1, 3, 8])
def test_hand_gradients_match_autograd(D, analytic):
  B = 5
  p, eps = _draw64(B, D, 20 + D)
  g = torch.randn(B, D, dtype=F64, generator=torch.Generator().manual_seed(3))
  fb = torch.tensor([1.0, 0.0, 1.0, -1.0, 1.0], dtype=F64)   # (clamped | capacity's sign among them)
  klw = 0.37
  pt = p.clone().requires_grad_(True)
  loc, _, L = tu.split(pt, D)
  kl = tu.kl_closed(loc, L) if analytic else tu.kl_mc(loc, L, eps)
  ((klw * fb * kl).sum() + (g * tu.sample(loc, L, eps)).sum()).backward()
  hand = tu.latent_bwd(p, eps, g, fb, klw, D, analytic)
  assert float((hand - pt.grad).abs().max()) <= 1e-9 * max(1.0, float(pt.grad.abs().max()))


def test_zero_off_diagonal_is_the_diagonal_closed_form():
  D, B = 6, 4
  p, _ = _draw64(B, D, 31)
  r = torch.zeros(B, tu.n_tril(D), dtype=F64)
  raw = p[:, D:2 * D]
  for i in range(D):
    r[:, tu.fill_index(i, i, D)] = raw[:, i]
  loc, _, L = tu.split(torch.cat([p[:, :D], r], -1), D)
  scale = (tu.softplus(raw) + 1e-5).numpy()
  assert np.abs(tu.kl_closed(loc, L).numpy() - vo.kl_analytic(p[:, :D].numpy(), scale)).max() <= 1e-9


# ---- 3. the kernels against float64 -------------------------------------------------------------------------------------
KERNEL_SIZES = [(1, 1), (3, 2), (5, 3), (7, 10), (4, 22), (2, 33), (64, 64), (9, 63)]


def draw32(B, D, seed):
  """float32 (p, eps): diagonal raws of -30 (L_ii -> 1e-5) and +30 (softplus is linear) in the first two samples"""
  rng = np.random.default_rng(seed)
  M = tu.n_tril(D)
  p = np.concatenate([rng.standard_normal((B, D)) * 0.7, rng.standard_normal((B, M)) * 0.5], 1)
  if B >= 2:
    p[0, D + tu.fill_index(0, 0, D)] = -30.0
    p[1, D + tu.fill_index(D - 1, D - 1, D)] = 30.0
  return p.astype(np.float32), rng.standard_normal((B, D)).astype(np.float32)


def run_fwd(bk, p, eps, D, analytic, free_bits=None, capacity=None):
  B = p.shape[0]
  z, kl, m = bk.zeros(B, D), bk.zeros(B), bk.zeros(B)
  pt, et = bk.T(p), bk.T(eps)
  cap = bk.T(np.array([capacity], np.float32)) if capacity is not None else None
  bk.L.odin_latent_tril_fwd(pt.data_ptr(), et.data_ptr(), z.data_ptr(), kl.data_ptr(), m.data_ptr(), B, D, int(analytic),
                            -1.0 if free_bits is None else float(free_bits), cap.data_ptr() if cap is not None else None,
                            None)
  sync(bk)
  return z.cpu().numpy(), kl.cpu().numpy(), m.cpu().numpy()


def run_bwd(bk, p, eps, z, dz, dzx, m, klw, D, analytic):
  B = p.shape[0]
  dp = bk.full(p.shape, float('nan'))
  w = bk.zeros(RANGE_WORDS, dtype=I32)
  ts = [bk.T(a) if a is not None else None for a in (p, eps, z, dz, dzx, m, np.array([klw], np.float32))]
  a = [t.data_ptr() if t is not None else None for t in ts]
  bk.L.odin_latent_tril_bwd(a[0], a[1], a[2], a[3], a[4], a[5], a[6], dp.data_ptr(), w.data_ptr(), B, D, int(analytic),
                            None)
  sync(bk)
  return dp.cpu().numpy(), float(w.cpu().view(torch.float32).max())


def thresholds(raw_kl, D):
  """-> [(free_bits, capacity)] for the case, from the float64 KL of the drawn batch: the free-bits threshold in the
  middle of the widest gap between two consecutive KL values, the capacity in the middle of the second widest (two
  samples: at three quarters of the one gap)"""
  s = np.sort(raw_kl)
  if len(s) == 1:
    return [(float(np.float32((max(s[0], 0.0) + 1.0) / D)), float(np.float32(s[0] - 0.7))),
            (float(np.float32(max(s[0], 0.2) / (2 * D))), float(np.float32(s[0] + 0.7)))]
  order = np.argsort(np.diff(s))[::-1]
  k = order[0]
  fb = float(np.float32(0.5 * (s[k] + s[k + 1]) / D))
  c = 0.25 * s[0] + 0.75 * s[1] if len(s) == 2 else 0.5 * (s[order[1]] + s[order[1] + 1])
  return [(fb, float(np.float32(c)))]


@pytest.mark.parametrize('analytic', [0, 1])
@pytest.mark.parametrize('B,D', KERNEL_SIZES)
def test_kernels_match_float64(bk, B, D, analytic):
  p, eps = draw32(B, D, 100 * B + D)
  rng = np.random.default_rng(B + D)
  dz = (rng.standard_normal((B, D)) * 0.3).astype(np.float32)
  dzx = (rng.standard_normal((B, D)) * 0.2).astype(np.float32)
  klw = float(np.float32(1.5 / B))
  raw = tu.latent_fwd(p, eps, D, analytic)[3].numpy()
  ths = thresholds(raw, D)
  kinds = set()
  for fb, cap in ths:
    thr = float(np.float32(fb)) * D
    # (a kernel inside the parity bound cannot move a sample across a threshold twice that bound away)
    margin = 2e-4 * max(1.0, np.abs(raw).max())
    assert thr > 0 and np.abs(raw - thr).min() > margin, 'a sample sits on the free-bits threshold'
    assert np.abs(raw - cap).min() > margin and abs(thr - cap) > margin, 'a sample sits on the capacity'
    kinds |= {bool(v) for v in (raw > thr)}
  assert kinds == {True, False}, 'the free-bits threshold must clamp some samples and spare others'
  for fb, cap in [(None, None)] + [(f, None) for f, _ in ths] + [(None, c) for _, c in ths] + ths:
    z64, kl64, m64, _ = tu.latent_fwd(p, eps, D, analytic, fb, cap)
    z, kl, m = run_fwd(bk, p, eps, D, analytic, fb, cap)
    close(z, z64.numpy())
    close(kl, kl64.numpy())
    assert np.array_equal(m, m64.numpy().astype(np.float32)), (fb, cap, m, m64)
    for extra in (None, dzx):
      g = dz.astype(np.float64) + (0.0 if extra is None else extra.astype(np.float64))
      ref = tu.latent_bwd(p, eps, g, m64.numpy(), klw, D, analytic).numpy()
      dp, word = run_bwd(bk, p, eps, z, dz, extra, m, klw, D, analytic)
      assert np.isfinite(dp).all()   # (every element written: the buffer started as NaN)
      close(dp, ref)
      assert word == float(np.abs(dp).max())
  # the decoder's gradient alone (no second input, no first input)
  dp0, _ = run_bwd(bk, p, eps, z, None, None, m, klw, D, analytic)
  close(dp0, tu.latent_bwd(p, eps, np.zeros((B, D)), m64.numpy(), klw, D, analytic).numpy())


def test_kernels_are_bit_reproducible(bk):
  B, D = 9, 63
  p, eps = draw32(B, D, 5)
  a, b = run_fwd(bk, p, eps, D, 0), run_fwd(bk, p, eps, D, 0)
  assert all(np.array_equal(x, y) for x, y in zip(a, b))
  dz = np.ones((B, D), np.float32)
  r1 = run_bwd(bk, p, eps, a[0], dz, None, a[2], 0.1, D, 0)
  r2 = run_bwd(bk, p, eps, a[0], dz, None, a[2], 0.1, D, 0)
  assert np.array_equal(r1[0], r2[0]) and r1[1] == r2[1]


def test_out_of_range_arguments_return_the_error_code(bk):
  B, D = 2, 65
  W = D + tu.n_tril(D)
  p, eps = bk.zeros(B, W), bk.zeros(B, D)
  outs = [bk.full((B, D), 7.0), bk.full((B,), 7.0), bk.full((B,), 7.0), bk.full((B, W), 7.0), bk.full((3 * B,), 7.0)]
  z, kl, m, dp, lq = outs
  one = bk.full((1,), 1.0)
  with pytest.raises(OdinError, match='D outside'):
    bk.L.odin_latent_tril_fwd(p.data_ptr(), eps.data_ptr(), z.data_ptr(), kl.data_ptr(), m.data_ptr(), B, D, 0, -1.0,
                              None, None)
  with pytest.raises(OdinError, match='D outside'):
    bk.L.odin_latent_tril_bwd(p.data_ptr(), eps.data_ptr(), z.data_ptr(), z.data_ptr(), None, m.data_ptr(),
                              one.data_ptr(), dp.data_ptr(), None, B, D, 0, None)
  with pytest.raises(OdinError, match='D outside'):
    bk.L.odin_latent_tril_sample_logprob(p.data_ptr(), eps.data_ptr(), z.data_ptr(), lq.data_ptr(), lq.data_ptr(), 1, B,
                                         D, None)
  for bad in (dict(B=0, D=4), dict(B=2, D=0)):
    with pytest.raises(OdinError):
      bk.L.odin_latent_tril_fwd(p.data_ptr(), eps.data_ptr(), z.data_ptr(), kl.data_ptr(), m.data_ptr(), bad['B'],
                                bad['D'], 0, -1.0, None, None)
  with pytest.raises(OdinError, match='analytic'):   # KL(p || q) is not offered
    bk.L.odin_latent_tril_fwd(p.data_ptr(), eps.data_ptr(), z.data_ptr(), kl.data_ptr(), m.data_ptr(), B, 4, 2, -1.0,
                              None, None)
  sync(bk)
  assert all(bool((t == 7.0).all()) for t in outs)


# ---- 4. odin_latent_tril_sample_logprob ---------------------------------------------------------------------------------
@pytest.mark.parametrize('n', [1, 3])
@pytest.mark.parametrize('B,D', [(5, 3), (2, 33), (3, 64)])
def test_sample_logprob_matches_float64(bk, n, B, D):
  p, _ = draw32(B, D, 7 * B + D)
  eps = np.random.default_rng(n).standard_normal((n, B, D)).astype(np.float32)
  z, lq, lp = bk.zeros(n, B, D), bk.zeros(n, B), bk.zeros(n, B)
  pt, et = bk.T(p), bk.T(eps)
  bk.L.odin_latent_tril_sample_logprob(pt.data_ptr(), et.data_ptr(), z.data_ptr(), lq.data_ptr(), lp.data_ptr(), n, B, D,
                                       None)
  sync(bk)
  loc, _, L = tu.split(p, D)
  e64 = torch.as_tensor(eps, dtype=F64)
  z64 = tu.sample(loc[None], L[None], e64)
  close(z.cpu().numpy(), z64.numpy())
  close(lq.cpu().numpy(), tu.log_q(L[None], e64).numpy())
  close(lp.cpu().numpy(), tu.log_p(z64).numpy())


def tril_nets(zdim=5, C=1):
  from odin_ai_amd.networks import RVconf
  nets = tiny_nets(C=C, zdim=zdim)
  nets['latents'] = RVconf(zdim, 'mvntril', projection=True, name='latents')
  return nets


def api_x(B=6, seed=2):
  return np.clip(np.random.default_rng(seed).random((B, 8, 8, 1)), 1e-6, 1 - 1e-6).astype(np.float32)


def test_marginal_log_prob_matches_float64_logmeanexp(bk):
  from odin_ai_amd.vae import VariationalAutoencoder
  from oracle.torch_ref import TorchVAE, t_seq
  D, n, N = 5, 3, 6
  vae = VariationalAutoencoder(device=bk.dev, lib=bk.L, **tril_nets(D))
  x = api_x(N)
  eps = np.random.default_rng(4).standard_normal((n, N, D)).astype(np.float32)
  llk, lat = vae.marginal_log_prob(x, n_mcmc=n, reduce=None, batch_size=4, eps=eps)
  T = {k: torch.as_tensor(v.cpu().numpy(), dtype=F64) for k, v in vae.trainable_variables.items()}
  x64 = torch.as_tensor(x, dtype=F64)
  h_e = t_seq(vae.encoder.layers, TorchVAE._sub(T, 'enc'), x64)
  loc, _, L = tu.split(h_e @ T[('lat', 'w')] + T[('lat', 'b')], D)
  e64 = torch.as_tensor(eps, dtype=F64)
  z = tu.sample(loc[None], L[None], e64)
  h_d = t_seq(vae.decoder.layers, TorchVAE._sub(T, 'dec'), z.reshape(n * N, D)).reshape((n, N, 8, 8, 1))
  lme = lambda t: (torch.logsumexp(t, 0) - math.log(n)).numpy()
  ref_llk = lme((x64[None] * h_d - tu.softplus(h_d)).reshape(n, N, -1).sum(-1))
  close(llk['image'].cpu().numpy(), ref_llk)
  close(lat['latents'][0].cpu().numpy(), lme(tu.log_q(L[None], e64)))
  close(lat['latents'][1].cpu().numpy(), lme(tu.log_p(z)))


# ---- 5. whole training steps against float64 autograd -------------------------------------------------------------------
def tril_case(bk, spec, B, seed=7, **engkw):
  """-> engine (latent_cov='tril'), its parameters as float64 arrays (the networks' through OracleVAE's initialiser, the
  projection drawn here: its shape is the new one), x, eps"""
  enc, dec, in_shape, D = spec
  eng = VAEEngine(enc, dec, in_shape, D, B, bk.dev, lib=bk.L, latent_cov='tril', **engkw)
  rng = np.random.default_rng(seed)
  P = vo.OracleVAE(enc, dec, in_shape, D, observation='bernoulli').init_params(seed=5)
  P = {k: np.asarray(v, np.float64) for k, v in P.items() if k[0] != 'lat'}
  P[('lat', 'w')] = (rng.standard_normal((eng.hdim, eng.pw)) * 0.2).astype(np.float32).astype(np.float64)
  P[('lat', 'b')] = (rng.standard_normal(eng.pw) * 0.1).astype(np.float32).astype(np.float64)
  eng.load_params(P)
  x = np.clip(rng.random((B,) + tuple(in_shape)), 1e-6, 1 - 1e-6).astype(np.float32)
  eps = rng.standard_normal((B, D)).astype(np.float32)
  return eng, P, x, eps


STEP_CASES = [('mc', dict(analytic=False), 1.5), ('analytic', dict(analytic=True), 0.4),
              ('mc_free_bits', dict(analytic=False, free_bits=0.9), 2.0),
              ('mmd', dict(analytic=False, latent_reg='mmd', reg_coef=3.0, mmd_prior_samples=7), 1.5)]


@pytest.mark.parametrize('cid,kw,beta', STEP_CASES, ids=[c[0] for c in STEP_CASES])
def test_three_train_steps_follow_float64_adam(bk, cid, kw, beta):
  spec, B, lr = tiny_spec(4), 6, 1e-3
  eng, P, x, eps = tril_case(bk, spec, B, hyper_ring_rows=16, **kw)
  assert eng.p.shape == (B, 4 + 10) and not (eng.lat_block or eng.neck)
  mmd = kw.get('latent_reg') == 'mmd'
  y = np.random.default_rng(9).standard_normal((7, 4)).astype(np.float32) if mmd else None
  ref = tu.TrilRef(spec[0], spec[1], 4, kw['analytic'], beta, kw.get('free_bits'), 3.0 if mmd else None)
  M = {k: np.zeros_like(v) for k, v in P.items()}
  V = {k: np.zeros_like(v) for k, v in P.items()}
  xt, et = bk.T(x), bk.T(eps)
  for t in (1, 2, 3):
    f, G, dp = ref.loss_and_grads(P, x, eps, y)
    out = eng.train_step(xt, et, lr=lr, beta=beta, prior=bk.T(y) if mmd else None).cpu().numpy()
    assert abs(out[0] - f['loss']) <= 1e-4 * max(1.0, abs(f['loss'])), (t, out[0], f['loss'])
    close(eng.kl.cpu().numpy(), f['kl'])
    close(eng.dp.cpu().numpy(), dp)   # the projection's gradient: of its output, its kernel and its bias
    gv = {k: v.cpu().numpy() for k, v in eng.grad_views().items()}
    assert set(gv) == set(G)
    for k in (('lat', 'w'), ('lat', 'b')):
      close(gv[k], G[k])
    _adam_ref(P, G, M, V, t, lr)
  got = {k: v.cpu().numpy() for k, v in eng.param_views().items()}
  assert set(got) == set(P) and got[('lat', 'w')].shape == (eng.hdim, 14)
  # every element of every parameter against the float64 trajectory
  for k in P:
    err, scale = float(np.abs(got[k] - P[k]).max()), max(1e-3, float(np.abs(P[k]).max()))
    print(f'{cid} {k}: max error {err:.3e} = {err / scale:.3e} of the largest weight')
    assert err <= 2e-4 * scale, (k, err, scale)


class TrilAudit(RangeAudit):
  """RangeAudit plus the two words of the triangular projection: h_e into the projection, dp out of the latent backward"""

  def _entries(self, eng):
    out = super()._entries(eng)
    if eng._tril_x_word is not None:
      out.append(('enc.outs[-1] -> projection', 'strict', eng._tril_x_word, eng.enc.outs[-1]))
    out.append(('dp -> projection gradients', 'strict', eng._tril_dp_word, eng.dp))
    return out


def wide_spec(D, width=256):
  """a Dense encoder of `width` units and no centring: the input's scale reaches the projection"""
  return ([('flatten',), ('dense', width, 'relu')],
          [('dense', 32, 'relu'), ('dense', 64, 'linear'), ('reshape', (8, 8, 1))], (8, 8, 1), D)


# D = 22 is the smallest D whose projection is at least 256 wide (256 -> 275).  The two-plane Dense kernels also want every width to
# be a multiple of 8, which 275 is not, so that case runs the fp32 family; D = 29 (256 -> 464) is the smallest D beyond it
# whose projection does run on the planes (asserted), with both of its range words read.
@pytest.mark.parametrize('D,planes', [(22, None), (29, True)])
def test_range_audit_wide_projection_scaled_inputs(bk, D, planes):
  B = 32 if planes else 8   # (the plane kernels start at 32 rows)
  eng, P, x, eps = tril_case(bk, wide_spec(D), B)
  assert eng.pw >= 256 and eng.hdim == 256
  if planes:
    assert eng._tril_x_word is not None and bk.L.odin_dense_reads_x_range(B, 256, eng.pw)
  audit = TrilAudit(eng)
  te = bk.T(eps)
  for scale in (1e5, 1e-30):
    eng.load_params(P)
    xs = (x.astype(np.float64) * scale).astype(np.float32)
    eng.train_step(bk.T(xs), te, lr=1e-3, beta=1.0, global_clipnorm=100.0)
    audit.check_cleared()
    assert bool(torch.isfinite(eng.out4).all()) and int(eng.flag.item()) == 0
    f, G, dp = tu.TrilRef(*wide_spec(D)[:2], D).loss_and_grads(P, xs, eps)
    assert abs(float(eng.out4[0]) - f['loss']) <= 1e-4 * max(1.0, abs(f['loss'])), (scale, float(eng.out4[0]), f['loss'])
    close(eng.dp.cpu().numpy(), dp)
    close(eng.enc.gouts[-1].cpu().numpy() * 1.0, _dh(P, f, dp))
  assert len(audit.steps) == 2 and not audit.failures
  names = [n for s in audit.steps for n, *_ in s]
  assert names.count('dp -> projection gradients') == 2
  audit.check_cover()


def _dh(P, f, dp):
  """d loss / d (pre-activation of the relu encoder layer) from the float64 dp"""
  return (dp @ P[('lat', 'w')].T) * (f['h_e'] > 0)


# ---- 6. engine behaviour ------------------------------------------------------------------------------------------------
def test_refused_combinations(bk):
  enc, dec, in_shape, zdim = tiny_spec()
  mk = lambda **kw: VAEEngine(enc, dec, in_shape, kw.pop('zdim', zdim), 4, bk.dev, lib=bk.L, latent_cov='tril', **kw)
  other = VAEEngine(enc, dec, in_shape, zdim, 4, bk.dev, lib=bk.L)
  for kw, exc, word in ((dict(tc='betatc'), ValueError, 'tc'), (dict(latent_reg='dip_i'), ValueError, 'dip_i'),
                        (dict(latent_reg='dip_ii'), ValueError, 'dip_ii'),
                        (dict(vamprior_components=3), ValueError, 'vamprior'),
                        (dict(vq_codes=5), ValueError, 'vq_codes'),
                        (dict(neck_bwd=True), NotImplementedError, 'neck_bwd'),
                        (dict(world_size=2), NotImplementedError, 'data parallel'),
                        (dict(force_dp=True), NotImplementedError, 'data parallel'),
                        (dict(range_words=other.range_words), NotImplementedError, 'range_words'),
                        (dict(analytic=True, reverse=False), NotImplementedError, 'reverse'),
                        (dict(zdim=65), ValueError, 'zdim')):
    with pytest.raises(exc, match=word):
      mk(**kw)
  with pytest.raises(ValueError, match='latent_cov'):
    VAEEngine(enc, dec, in_shape, zdim, 4, bk.dev, lib=bk.L, latent_cov='full')
  eng = mk(latent_reg='mmd')
  with pytest.raises(NotImplementedError, match='reverse'):
    eng.set_kl_form(True, reverse=False)


def test_fused_forms_are_ignored_under_tril(bk):
  spec = neck_spec(5, 128)
  assert VAEEngine(*spec, 2, bk.dev, lib=bk.L, neck=True).neck
  calls = []
  eng = VAEEngine(*spec, 2, bk.dev, lib=Recorder(bk.L, calls), neck=True, latent_cov='tril')
  assert not (eng.neck or eng.lat_block)
  x, eps = case_data(bk.dev, spec, B=2)
  calls.clear()
  eng.train_step(x, eps, lr=1e-3, beta=2.0)   # (forward(fused=True): the default)
  assert not [c for c in calls if 'neck' in c or 'latent_block' in c or c in ('odin_latent_fwd', 'odin_latent_bwd')]
  assert calls.count('odin_latent_tril_fwd') == 1 and calls.count('odin_latent_tril_bwd') == 1
  assert calls.index('odin_latent_tril_fwd') < calls.index('odin_latent_tril_bwd')
  assert bool(torch.isfinite(eng.out4).all())


def test_plain_engine_call_list_is_unchanged(bk):
  eng, c1 = launch_record(bk)
  assert c1 == PLAIN_STEP_CALLS and eng.latent_cov == 'diag' and eng.pw == 2 * eng.D
  _, c2 = launch_record(bk, latent_cov='diag')
  assert c2 == PLAIN_STEP_CALLS
  nl = len(eng.enc_recs) + len(eng.dec_recs)
  assert eng.range_words.numel() == 2 * nl * RANGE_WORDS


@pytest.mark.gpu
def test_graph_replay_over_a_beta_schedule_equals_eager():
  """four steps under beta = 0.5, 1, 2, 4: the captured step replays bit for bit what the eager launches compute -- klw
  is read from device memory (the simulator has no graphs: GPU only, like the other models' replay tests)"""
  from tests.test_latent_regularizers import _Hip
  bk = _Hip()
  res = []
  for use_graph in (False, True):
    eng, P, x, eps = tril_case(bk, tiny_spec(4), 6)
    xt = bk.T(x)
    outs = [eng.train_step(xt, None, lr=1e-3, beta=b, use_graph=use_graph).clone() for b in (0.5, 1.0, 2.0, 4.0)]
    sync(bk)
    res.append([eng.params.clone(), torch.stack(outs), eng.dp.clone(), eng.z.clone()])
  for a, b in zip(res[0], res[1]):
    assert torch.equal(a, b)
  kls = res[0][1][:, 2]
  assert bool(torch.isfinite(res[0][1]).all()) and len(set(kls.tolist())) == 4


# ---- 7. the model API ---------------------------------------------------------------------------------------------------
def test_api_quick_start_builds_fits_and_returns_the_posterior(bk):
  from odin_ai_amd.vae import BetaVAE, MVNTriLPosterior
  vae = BetaVAE(beta=2.0, device=bk.dev, lib=bk.L, **tril_nets(5))
  x = api_x(8)
  before, _ = vae.optimize(x, training=False)
  vae.fit(x, max_iter=3, batch_size=8, learning_rate=1e-3, compile_graph=False)
  assert vae.step == 3 and np.isfinite(float(vae.optimize(x, training=False)[0])) and np.isfinite(float(before))
  px, qz = vae(x)
  assert isinstance(qz, MVNTriLPosterior) and qz.event_shape == (5,) and qz.batch_shape == (8,)
  L = qz.scale_tril
  assert L.shape == (8, 5, 5) and bool((torch.triu(L, 1) == 0).all()) and float(torch.diagonal(L, dim1=1, dim2=2).min()) > 0
  assert torch.allclose(qz.covariance(), L @ L.transpose(1, 2), rtol=0, atol=1e-6)
  assert torch.allclose(qz.stddev(), torch.sqrt(torch.diagonal(qz.covariance(), dim1=1, dim2=2)), rtol=1e-5, atol=1e-7)
  assert torch.equal(qz.mean(), qz.loc) and qz.sample(3, seed=1).shape == (3, 8, 5)
  # the posterior's own numbers against the restatement (p = loc | raw as the engine left it)
  p64 = torch.cat([qz.loc, qz.raw_scale], 1).cpu().numpy().astype(np.float64)
  loc, _, L64 = tu.split(p64, 5)
  close(L.cpu().numpy(), L64.numpy(), 1e-6)
  z = qz.tensor()
  e64 = torch.linalg.solve_triangular(L64, (torch.as_tensor(z.cpu().numpy(), dtype=F64) - loc)[..., None], upper=False)[..., 0]
  close(qz.log_prob(z).cpu().numpy(), tu.log_q(L64, e64).numpy())
  close(qz.KL_divergence(analytic=True).cpu().numpy(), tu.kl_closed(loc, L64).numpy())
  close(qz.KL_divergence(analytic=False).cpu().numpy(), tu.kl_mc(loc, L64, e64).numpy())
  with pytest.raises(NotImplementedError, match='reverse'):
    qz.KL_divergence(analytic=True, reverse=False)
  # elbo_components: the engine's KL (times beta) is the wrapper's KL at the engine's sample
  eps = np.random.default_rng(1).standard_normal((8, 5)).astype(np.float32)
  llk, kl = vae.elbo_components(x, eps=eps)
  _, q2 = vae.last_outputs
  close(kl['kl_latents'].cpu().numpy(), 2.0 * q2.KL_divergence(analytic=False).cpu().numpy())
  assert vae.sample_prior(4).shape == (4, 5) and vae.trainable_variables[('lat', 'w')].shape == (24, 20)
  assert vae.variable_name(('lat', 'w')) == 'latents/kernel'


@pytest.mark.parametrize('fmt', ['npz', 'tf'])
def test_api_save_load_round_trip(bk, tmp_path, fmt):
  from odin_ai_amd.vae import BetaVAE
  vae = BetaVAE(beta=2.0, device=bk.dev, lib=bk.L, **tril_nets(5))
  x = api_x()
  vae.optimize(x, learning_rate=1e-2)
  path = str(tmp_path / 'w')
  vae.save_weights(path, save_format=fmt)
  other = BetaVAE(beta=2.0, device=bk.dev, lib=bk.L, seed=3, **tril_nets(5))
  assert not torch.equal(other.trainable_variables[('lat', 'w')], vae.trainable_variables[('lat', 'w')])
  other.load_weights(path, raise_notfound=True)
  assert other.step == 1
  for k, v in vae.trainable_variables.items():
    assert torch.equal(v, other.trainable_variables[k]), k
  eps = np.random.default_rng(1).standard_normal((6, 5)).astype(np.float32)
  a, b = vae.elbo_components(x, eps=eps), other.elbo_components(x, eps=eps)
  assert torch.equal(a[0]['llk_image'], b[0]['llk_image']) and torch.equal(a[1]['kl_latents'], b[1]['kl_latents'])


def test_api_supported_and_refused_classes(bk):
  from odin_ai_amd.networks import get_networks
  from odin_ai_amd.vae import get_vae
  x = api_x()
  for name, kw in (('vae', {}), ('betavae', dict(beta=2.0)), ('annealingvae', {}), ('betacapacityvae', {}),
                   ('infovae', dict(alpha=0.2, lamda=5.0))):
    vae = get_vae(name)(device=bk.dev, lib=bk.L, **kw, **tril_nets(5))
    loss, metrics = vae.optimize(x, learning_rate=1e-3)
    assert np.isfinite(float(loss)) and vae._engine(6).latent_cov == 'tril', name
  for name in ('betatcvae', 'dipvae', 'vampriorvae', 'vqvae', 'factorvae'):
    with pytest.raises(ValueError, match='mvntril'):
      get_vae(name)(device=bk.dev, lib=bk.L, **tril_nets(5))
  vae = get_vae('vae')(device=bk.dev, lib=bk.L, analytic=True, free_bits=0.3, sample_shape=(2,), **tril_nets(5))
  llk, kl = vae.elbo_components(x)
  assert llk['llk_image'].shape == (2, 6) and kl['kl_latents'].shape == (1, 6)
  assert float(kl['kl_latents'].min()) >= 0.3 * 5 - 1e-6
  with pytest.raises(NotImplementedError, match='reverse'):
    vae.set_elbo_configs(reverse=False)
  with pytest.raises(NotImplementedError, match='reverse'):
    get_vae('vae')(device=bk.dev, lib=bk.L, analytic=True, reverse=False, **tril_nets(5))
  assert get_networks('dsprites', qz='mvntril')['latents'].posterior == 'mvntril'


# ---- 8. full size on the MI355X -----------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize('D,proj,analytic', [(10, 128, False), (29, 256, True)], ids=['dsprites_d10', 'planes_d29'])
def test_gpu_full_size_step(D, proj, analytic):
  """the dSprites stack at batch 256, one step against float64 autograd; D = 29 under a 256-wide encoder puts the
  projection (256 -> 464) on the two-plane Dense kernels with both of its range words"""
  from tests.test_latent_regularizers import _Hip
  bk = _Hip()
  spec = vo.dsprites_spec(1, zdim=D, proj_dim=proj)
  eng, P, x, eps = tril_case(bk, spec, 256, analytic=analytic)
  assert (eng._tril_x_word is not None) == (D == 29)
  eng.step_count = 1
  eng.set_hyper(beta=1.5)
  eng.forward(bk.T(x), bk.T(eps))
  eng.backward()
  torch.cuda.synchronize()
  f, G, dp = tu.TrilRef(spec[0], spec[1], D, analytic, 1.5).loss_and_grads(P, x, eps)
  out4 = eng.out4.cpu().numpy()
  assert abs(out4[0] - f['loss']) <= 1e-4 * max(1.0, abs(f['loss'])), (out4[0], f['loss'])
  close(eng.llk.cpu().numpy(), f['llk'])
  close(eng.kl.cpu().numpy(), f['kl'])
  close(eng.z.cpu().numpy(), f['z'])
  close(eng.dp.cpu().numpy(), dp)
  gv = {k: v.cpu().numpy() for k, v in eng.grad_views().items()}
  assert set(gv) == set(G)
  for k in G:
    close(gv[k], G[k])
