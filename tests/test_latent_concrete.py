"""The relaxed one-hot (Concrete / Gumbel-softmax) posterior 'relaxedonehot' (latent_concrete.hip,
VAEEngine(latent_dist='relaxedonehot'), RelaxedOneHotPosterior) on both backends of the `bk` fixture: the float64
restatement of tests/concrete_util.py against torch's own RelaxedOneHotCategorical / Categorical and autograd, the Gumbel
stream, the kernels against that restatement, whole training steps against float64 autograd, the engine's behaviour and
the model API.

Tolerances: 1e-4 of a tensor's maximum for values and gradients (the project's parity bound); the restatement against
torch.distributions to 1e-9; fbmask and everything the kernels promise bit for bit, exactly.

Free bits "clamp some but not all samples": the threshold (and the capacity) lies in the middle of the (second) widest
gap between two KL values of the drawn batch, as tests/test_latent_tril.py places it (asserted: both kinds occur, and no
sample sits within twice the parity bound of a threshold).  A batch of ONE sample cannot hold both kinds: there the
kernel runs once under a threshold above the sample's KL and once under one below it.

The Gumbel stream's moments over n = 200 001: mean within 0.015 of Euler's constant, variance within 0.04 of pi^2 / 6
-- five standard errors of either estimate at this n (sd of the mean 1.28 / sqrt(n) = 0.0029; of the variance
sqrt((mu4 - sigma^4) / n) = 0.0082 with the Gumbel's mu4 = 5.4 sigma^4).

Whole steps: the loss and the projection's gradient at the parity bound; every element of every parameter after three
Adam steps to 2e-4 of its tensor's largest weight, the bar of the other models' step tests (tests/test_vq.py)."""
import math

import numpy as np
import pytest
import torch

from odin_ai_amd._lib import OdinError
from odin_ai_amd.engine import RANGE_WORDS, VAEEngine
from oracle import vae_oracle as vo
from tests import concrete_util as cu
from tests.engine_util import Recorder, case_data, launch_record, neck_spec, tiny_nets, tiny_spec
from tests.test_latent_regularizers import _adam_ref
from tests.test_vamprior import PLAIN_STEP_CALLS

F64 = torch.float64
EULER = 0.5772156649015329


def close(got, ref, tol=1e-4):
  got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
  scale = max(float(np.abs(ref).max()), 1e-30)
  err = float(np.abs(got - ref).max())
  assert err <= tol * scale, (err, scale)


def sync(bk):
  if bk.dev.type == 'cuda':
    torch.cuda.synchronize()


# ---- 1. the restatement against torch's own distributions --------------------------------------------------------------
def _draw64(B, K, seed, std=1.0):
  gen = torch.Generator().manual_seed(seed)
  l = torch.randn(B, K, generator=gen, dtype=F64) * std
  u = torch.rand(B, K, generator=gen, dtype=F64).clamp(1e-12, 1 - 1e-12)
  return l, -torch.log(-torch.log(u))


@pytest.mark.parametrize('tau', [0.1, 0.5, 1.0])
@pytest.mark.parametrize('K', [2, 3, 10, 64])
def test_restatement_matches_torch_distributions(K, tau):
  from torch.distributions import Categorical, RelaxedOneHotCategorical, kl_divergence
  l, g = _draw64(6, K, 10 + K)
  y, z = cu.relax(l, g, tau)
  ref = RelaxedOneHotCategorical(torch.tensor(tau, dtype=F64), logits=l).log_prob(z)
  tol = dict(rtol=0, atol=1e-9)
  assert torch.allclose(cu.log_q(l, y, tau), ref, **tol)
  assert torch.allclose(cu.log_q_noise(g, y, tau), ref, **tol)
  assert torch.allclose(z.sum(-1), torch.ones(6, dtype=F64), **tol)
  assert torch.allclose(cu.log_p(z), torch.full((6,), -math.log(K), dtype=F64), **tol)
  uniform = Categorical(logits=torch.zeros(K, dtype=F64))
  assert torch.allclose(cu.kl_categorical(l), kl_divergence(Categorical(logits=l), uniform), **tol)


@pytest.mark.parametrize('analytic', [False, True])
@pytest.mark.parametrize('tau', [0.1, 0.5, 1.0])
@pytest.mark.parametrize('K', [2, 3, 10, 64])
def test_hand_gradients_match_autograd(K, tau, analytic):
  B = 5
  l, g = _draw64(B, K, 20 + K)
  G = torch.randn(B, K, dtype=F64, generator=torch.Generator().manual_seed(3))
  fb = torch.tensor([1.0, 0.0, 1.0, -1.0, 1.0], dtype=F64)   # (clamped | capacity's sign among them)
  klw = 0.37
  lt = l.clone().requires_grad_(True)
  kl = cu.kl_categorical(lt) if analytic else cu.kl_mc(lt, g, tau)
  ((klw * fb * kl).sum() + (G * cu.relax(lt, g, tau)[1]).sum()).backward()
  hand = cu.latent_bwd(l, g, G, fb, klw, tau, analytic)
  assert float((hand - lt.grad).abs().max()) <= 1e-9 * max(1.0, float(lt.grad.abs().max()))


# ---- 2. the Gumbel stream -----------------------------------------------------------------------------------------------
def rng_gumbel(bk, n, seed, step=None):
  out = bk.full((n,), float('nan'))
  st = bk.T(np.array([step]), torch.int32) if step is not None else None
  bk.L.odin_rng_gumbel(out.data_ptr(), n, seed, st.data_ptr() if st is not None else None, None)
  sync(bk)
  return out.cpu().numpy()


def test_rng_gumbel_stream(bk):
  n = 200001
  a, b, c = rng_gumbel(bk, n, 11, 4), rng_gumbel(bk, n, 11, 4), rng_gumbel(bk, n, 11, 5)
  assert np.array_equal(a, b) and not np.array_equal(a, c)
  assert np.array_equal(rng_gumbel(bk, n, 11), rng_gumbel(bk, n, 11, 0))   # (no step word: step 0)
  assert np.isfinite(a).all() and a.min() >= -2.86 and a.max() <= 17.33
  a64 = a.astype(np.float64)
  print(f'gumbel stream: mean - gamma = {a64.mean() - EULER:+.5f}, var - pi^2/6 = {a64.var() - math.pi ** 2 / 6:+.5f}')
  assert abs(a64.mean() - EULER) <= 0.015
  assert abs(a64.var() - math.pi ** 2 / 6) <= 0.04


def run_fwd(bk, p, g, tau, analytic, free_bits=None, capacity=None, draw=None):
  """draw: None (the noise g is read) | (seed, step): drawn in the kernel; -> z, kl, fbmask, the noise buffer"""
  B, K = p.shape
  z, kl, m = bk.zeros(B, K), bk.zeros(B), bk.zeros(B)
  pt = bk.T(p)
  gt = bk.T(g) if draw is None else bk.full((B, K), float('nan'))
  cap = bk.T(np.array([capacity], np.float32)) if capacity is not None else None
  st = bk.T(np.array([draw[1]]), torch.int32) if draw is not None else None
  bk.L.odin_latent_concrete_fwd(pt.data_ptr(), gt.data_ptr(), z.data_ptr(), kl.data_ptr(), m.data_ptr(), B, K, float(tau),
                                int(analytic), -1.0 if free_bits is None else float(free_bits),
                                cap.data_ptr() if cap is not None else None, int(draw is not None),
                                draw[0] if draw is not None else 0, st.data_ptr() if st is not None else None, None)
  sync(bk)
  return z.cpu().numpy(), kl.cpu().numpy(), m.cpu().numpy(), gt.cpu().numpy()


@pytest.mark.parametrize('B,K', [(6, 10), (5, 3)])   # (15 elements: no multiple of the counter's 4)
def test_forward_draws_the_gumbel_stream_bit_for_bit(bk, B, K):
  p = (np.random.default_rng(B).standard_normal((B, K)) * 1.5).astype(np.float32)
  stream = rng_gumbel(bk, B * K, 2 ** 33 + 5, 9).reshape(B, K)
  z, kl, m, g = run_fwd(bk, p, None, 0.5, 0, draw=(2 ** 33 + 5, 9))
  assert np.array_equal(g, stream)
  # and the sample is the one the explicit noise gives
  z2, kl2, m2, _ = run_fwd(bk, p, stream, 0.5, 0)
  assert np.array_equal(z, z2) and np.array_equal(kl, kl2) and np.array_equal(m, m2)
  close(z, cu.latent_fwd(p, stream, 0.5, 0)[0].numpy())


# ---- 3. the kernels against float64 -------------------------------------------------------------------------------------
KERNEL_SIZES = [(1, 2), (5, 3), (6, 10), (9, 64), (257, 7)]   # one sample | a partial last workgroup | a full wave | 65 workgroups


def draw32(B, K, seed, std=1.5):
  """float32 (logits, Gumbel noise)"""
  rng = np.random.default_rng(seed)
  return (rng.standard_normal((B, K)) * std).astype(np.float32), rng.gumbel(size=(B, K)).astype(np.float32)


def run_bwd(bk, p, g, z, dz, dzx, m, klw, tau, analytic):
  B, K = p.shape
  dp = bk.full(p.shape, float('nan'))
  ts = [bk.T(a) if a is not None else None for a in (p, g, z, dz, dzx, m, np.array([klw], np.float32))]
  a = [t.data_ptr() if t is not None else None for t in ts]
  bk.L.odin_latent_concrete_bwd(a[0], a[1], a[2], a[3], a[4], a[5], a[6], dp.data_ptr(), B, K, float(tau), int(analytic),
                                None)
  sync(bk)
  return dp.cpu().numpy()


def thresholds(raw_kl, K):
  """-> [(free_bits, capacity)] for the case, from the float64 KL of the drawn batch: the free-bits threshold in the
  middle of the widest gap between two consecutive KL values, the capacity in the middle of the second widest (two
  samples: at three quarters of the one gap); ONE sample: a threshold above its KL, then one below it"""
  s = np.sort(raw_kl)
  if len(s) == 1:
    assert s[0] > 0.2, 'the single sample needs a KL a positive threshold fits under'
    return [(float(np.float32((s[0] + 1.0) / K)), float(np.float32(s[0] - 0.7))),
            (float(np.float32(s[0] / (2 * K))), float(np.float32(s[0] + 0.7)))]
  order = np.argsort(np.diff(s))[::-1]
  k = order[0]
  fb = float(np.float32(0.5 * (s[k] + s[k + 1]) / K))
  c = 0.25 * s[0] + 0.75 * s[1] if len(s) == 2 else 0.5 * (s[order[1]] + s[order[1] + 1])
  return [(fb, float(np.float32(c)))]


@pytest.mark.parametrize('analytic', [0, 1])
@pytest.mark.parametrize('B,K', KERNEL_SIZES)
def test_kernels_match_float64(bk, B, K, analytic):
  tau = 0.5
  p, g = draw32(B, K, 100 * B + K)
  rng = np.random.default_rng(B + K)
  dz = (rng.standard_normal((B, K)) * 0.3).astype(np.float32)
  dzx = (rng.standard_normal((B, K)) * 0.2).astype(np.float32)
  klw = float(np.float32(1.5 / B))
  raw = cu.latent_fwd(p, g, tau, analytic)[3].numpy()
  ths = thresholds(raw, K)
  kinds = set()
  for fb, cap in ths:
    thr = float(np.float32(fb)) * K
    # (a kernel inside the parity bound cannot move a sample across a threshold twice that bound away)
    margin = 2e-4 * max(1.0, np.abs(raw).max())
    assert thr > 0 and np.abs(raw - thr).min() > margin, 'a sample sits on the free-bits threshold'
    assert np.abs(raw - cap).min() > margin and abs(thr - cap) > margin, 'a sample sits on the capacity'
    kinds |= {bool(v) for v in (raw > thr)}
  assert kinds == {True, False}, 'the free-bits threshold must clamp some samples and spare others'
  for fb, cap in [(None, None)] + [(f, None) for f, _ in ths] + [(None, c) for _, c in ths] + ths:
    z64, kl64, m64, _ = cu.latent_fwd(p, g, tau, analytic, fb, cap)
    z, kl, m, _ = run_fwd(bk, p, g, tau, analytic, fb, cap)
    close(z, z64.numpy())
    close(kl, kl64.numpy())
    assert np.array_equal(m, m64.numpy().astype(np.float32)), (fb, cap, m, m64)
    for extra in (None, dzx):
      G = dz.astype(np.float64) + (0.0 if extra is None else extra.astype(np.float64))
      ref = cu.latent_bwd(p, g, G, m64.numpy(), klw, tau, analytic).numpy()
      dp = run_bwd(bk, p, g, z, dz, extra, m, klw, tau, analytic)
      assert np.isfinite(dp).all()   # (every element written: the buffer started as NaN)
      close(dp, ref)
  # the KL's gradient alone (neither input), and without the noise buffer, which the gradients do not read
  dp0 = run_bwd(bk, p, None, z, None, None, m, klw, tau, analytic)
  close(dp0, cu.latent_bwd(p, g, np.zeros((B, K)), m64.numpy(), klw, tau, analytic).numpy())


def run_sample_logprob(bk, p, g, tau):
  n, B, K = g.shape
  z, lq, lp = bk.zeros(n, B, K), bk.zeros(n, B), bk.zeros(n, B)
  pt, gt = bk.T(p), bk.T(g)
  bk.L.odin_latent_concrete_sample_logprob(pt.data_ptr(), gt.data_ptr(), z.data_ptr(), lq.data_ptr(), lp.data_ptr(), n, B,
                                           K, float(tau), None)
  sync(bk)
  return z.cpu().numpy(), lq.cpu().numpy(), lp.cpu().numpy()


def test_low_temperature_underflow_stays_finite(bk):
  """tau = 0.1, K = 10, logits of standard deviation 2: z underflows to exactly 0 in float32 (y below -104, under the
  smallest denormal), and everything that is computed in y stays finite and at the parity bound"""
  tau, B, K = 0.1, 16, 10
  p, g = draw32(B, K, 3, std=2.0)
  y64, z64 = cu.relax(cu.t64(p), cu.t64(g), tau)
  assert float(y64.min()) < -110.0   # (the seed was chosen for this)
  for analytic in (0, 1):
    z, kl, m, _ = run_fwd(bk, p, g, tau, analytic)
    assert (z == 0.0).any() and np.isfinite(z).all() and np.isfinite(kl).all()
    _, kl64, m64, _ = cu.latent_fwd(p, g, tau, analytic)
    close(z, z64.numpy())
    close(kl, kl64.numpy())
    rng = np.random.default_rng(1)
    dz = (rng.standard_normal((B, K)) * 0.3).astype(np.float32)
    dp = run_bwd(bk, p, g, z, dz, None, m, 0.25, tau, analytic)
    assert np.isfinite(dp).all()
    close(dp, cu.latent_bwd(p, g, dz, m64.numpy(), 0.25, tau, analytic).numpy())
  zs, lq, lp = run_sample_logprob(bk, p, g[None], tau)
  assert np.isfinite(lq).all() and np.array_equal(zs[0], z)
  close(lq[0], cu.log_q(cu.t64(p), y64, tau).numpy())
  close(lp[0], cu.log_p(z64).numpy())


@pytest.mark.parametrize('B,K,tau', [(5, 3, 0.5), (3, 64, 1.0), (6, 10, 0.1)])
def test_sample_logprob_matches_float64(bk, B, K, tau):
  n = 3
  p, _ = draw32(B, K, 7 * B + K)
  g = np.random.default_rng(n).gumbel(size=(n, B, K)).astype(np.float32)
  z, lq, lp = run_sample_logprob(bk, p, g, tau)
  l64, g64 = cu.t64(p)[None].expand(n, B, K), cu.t64(g)
  y64, z64 = cu.relax(l64, g64, tau)
  close(z, z64.numpy())
  close(lq, cu.log_q(l64, y64, tau).numpy())
  close(lp, cu.log_p(z64).numpy())


def test_kernels_are_bit_reproducible(bk):
  p, g = draw32(9, 63, 5)
  a, b = run_fwd(bk, p, g, 0.5, 0), run_fwd(bk, p, g, 0.5, 0)
  assert all(np.array_equal(x, y) for x, y in zip(a, b))
  dz = np.ones((9, 63), np.float32)
  r1 = run_bwd(bk, p, g, a[0], dz, None, a[2], 0.1, 0.5, 0)
  r2 = run_bwd(bk, p, g, a[0], dz, None, a[2], 0.1, 0.5, 0)
  assert np.array_equal(r1, r2)


def test_out_of_range_arguments_return_the_error_code(bk):
  B = 2
  p, g = bk.zeros(B, 65), bk.zeros(3 * B, 65)
  outs = [bk.full((3 * B, 65), 7.0), bk.full((B,), 7.0), bk.full((B,), 7.0), bk.full((B, 65), 7.0), bk.full((3 * B,), 7.0)]
  z, kl, m, dp, lq = outs
  one = bk.full((1,), 1.0)
  for K, tau, analytic, word in ((1, 0.5, 0, 'K outside'), (65, 0.5, 0, 'K outside'), (4, 0.0, 0, 'temperature'),
                                 (4, -1.0, 0, 'temperature'), (4, 0.5, 2, 'analytic')):
    for draw in (0, 1):
      with pytest.raises(OdinError, match=word) as e:
        bk.L.odin_latent_concrete_fwd(p.data_ptr(), g.data_ptr(), z.data_ptr(), kl.data_ptr(), m.data_ptr(), B, K, tau,
                                      analytic, -1.0, None, draw, 1, None, None)
      assert 'rc=-2' in str(e.value)
    with pytest.raises(OdinError, match=word) as e:
      bk.L.odin_latent_concrete_bwd(p.data_ptr(), g.data_ptr(), z.data_ptr(), z.data_ptr(), None, m.data_ptr(),
                                    one.data_ptr(), dp.data_ptr(), B, K, tau, analytic, None)
    assert 'rc=-2' in str(e.value)
    if analytic == 0:
      with pytest.raises(OdinError, match=word) as e:
        bk.L.odin_latent_concrete_sample_logprob(p.data_ptr(), g.data_ptr(), z.data_ptr(), lq.data_ptr(), lq.data_ptr(),
                                                 3, B, K, tau, None)
      assert 'rc=-2' in str(e.value)
  with pytest.raises(OdinError, match='batch'):
    bk.L.odin_latent_concrete_fwd(p.data_ptr(), g.data_ptr(), z.data_ptr(), kl.data_ptr(), m.data_ptr(), 0, 4, 0.5, 0,
                                  -1.0, None, 0, 1, None, None)
  sync(bk)
  assert all(bool((t == 7.0).all()) for t in outs) and bool((g == 0.0).all())


# ---- 4. whole training steps against float64 autograd -------------------------------------------------------------------
def concrete_case(bk, spec, B, seed=7, **engkw):
  """-> engine (latent_dist='relaxedonehot'), its parameters as float64 arrays (the networks' through OracleVAE's
  initialiser, the projection drawn here: its shape is the new one), x, the Gumbel noise"""
  enc, dec, in_shape, K = spec
  eng = VAEEngine(enc, dec, in_shape, K, B, bk.dev, lib=bk.L, latent_dist='relaxedonehot', **engkw)
  rng = np.random.default_rng(seed)
  P = vo.OracleVAE(enc, dec, in_shape, K, observation='bernoulli').init_params(seed=5)
  P = {k: np.asarray(v, np.float64) for k, v in P.items() if k[0] != 'lat'}
  P[('lat', 'w')] = (rng.standard_normal((eng.hdim, K)) * 0.3).astype(np.float32).astype(np.float64)
  P[('lat', 'b')] = (rng.standard_normal(K) * 0.1).astype(np.float32).astype(np.float64)
  eng.load_params(P)
  x = np.clip(rng.random((B,) + tuple(in_shape)), 1e-6, 1 - 1e-6).astype(np.float32)
  return eng, P, x, rng.gumbel(size=(B, K)).astype(np.float32)


# (free bits of 1.3 per category: 6.5 nats, between the KL values of the batch -- asserted below)
STEP_CASES = [('mc', dict(analytic=False), 1.5), ('analytic', dict(analytic=True), 0.4),
              ('mc_free_bits', dict(analytic=False, free_bits=1.3), 2.0)]


@pytest.mark.parametrize('cid,kw,beta', STEP_CASES, ids=[c[0] for c in STEP_CASES])
def test_three_train_steps_follow_float64_adam(bk, cid, kw, beta):
  spec, B, K, lr = tiny_spec(5), 6, 5, 1e-3
  eng, P, x, g = concrete_case(bk, spec, B, hyper_ring_rows=16, **kw)
  assert eng.p.shape == (B, K) and eng.dp.shape == (B, K) and eng.eps.shape == (B, K) and not (eng.lat_block or eng.neck)
  ref = cu.ConcreteRef(spec[0], spec[1], K, 0.5, kw['analytic'], beta, kw.get('free_bits'))
  M = {k: np.zeros_like(v) for k, v in P.items()}
  V = {k: np.zeros_like(v) for k, v in P.items()}
  xt, gt = bk.T(x), bk.T(g)
  for t in (1, 2, 3):
    f, G, dp = ref.loss_and_grads(P, x, g)
    if t == 1 and 'free_bits' in kw:
      hit = f['kl'] <= kw['free_bits'] * K + 1e-12
      assert hit.any() and not hit.all(), f['kl']
    out = eng.train_step(xt, gt, lr=lr, beta=beta).cpu().numpy()
    assert abs(out[0] - f['loss']) <= 1e-4 * max(1.0, abs(f['loss'])), (t, out[0], f['loss'])
    close(eng.kl.cpu().numpy(), f['kl'])
    close(eng.dp.cpu().numpy(), dp)   # the projection's gradient: of its output, its kernel and its bias
    gv = {k: v.cpu().numpy() for k, v in eng.grad_views().items()}
    assert set(gv) == set(G)
    for k in (('lat', 'w'), ('lat', 'b')):
      close(gv[k], G[k])
    _adam_ref(P, G, M, V, t, lr)
  got = {k: v.cpu().numpy() for k, v in eng.param_views().items()}
  assert set(got) == set(P) and got[('lat', 'w')].shape == (eng.hdim, K) and got[('lat', 'b')].shape == (K,)
  # every element of every parameter against the float64 trajectory
  for k in P:
    err, scale = float(np.abs(got[k] - P[k]).max()), max(1e-3, float(np.abs(P[k]).max()))
    print(f'{cid} {k}: max error {err:.3e} = {err / scale:.3e} of the largest weight')
    assert err <= 2e-4 * scale, (k, err, scale)


@pytest.mark.gpu
def test_graph_replay_over_a_beta_schedule_equals_eager():
  """four steps under beta = 0.5, 1, 2, 4 with the noise drawn in the kernel: the captured step replays bit for bit what
  the eager launches compute -- klw and the step are read from device memory (the simulator has no graphs: GPU only, like
  the other models' replay tests)"""
  from tests.test_latent_regularizers import _Hip
  bk = _Hip()
  res = []
  for use_graph in (False, True):
    eng, P, x, g = concrete_case(bk, tiny_spec(5), 6)
    xt = bk.T(x)
    outs = [eng.train_step(xt, None, lr=1e-3, beta=b, use_graph=use_graph).clone() for b in (0.5, 1.0, 2.0, 4.0)]
    sync(bk)
    res.append([eng.params.clone(), torch.stack(outs), eng.dp.clone(), eng.z.clone(), eng.eps.clone()])
  for a, b in zip(res[0], res[1]):
    assert torch.equal(a, b)
  klb = res[0][1][:, 2]   # (mean beta * kl: another noise and another beta at every step)
  assert bool(torch.isfinite(res[0][1]).all()) and len(set(klb.tolist())) == 4
  # a beta change between two replays of the SAME noise is seen: the KL term scales, the likelihood's does not
  eng, P, x, g = concrete_case(bk, tiny_spec(5), 6)
  xt, gt = bk.T(x), bk.T(g)
  o1 = eng.train_step(xt, gt, lr=0.0, beta=1.0, use_graph=True).clone()
  o2 = eng.train_step(xt, gt, lr=0.0, beta=3.0, use_graph=True).clone()
  assert float(o1[1]) == float(o2[1]) and abs(float(o2[2]) - 3.0 * float(o1[2])) <= 1e-5 * abs(float(o2[2]))


# ---- 5. engine behaviour ------------------------------------------------------------------------------------------------
def test_refused_combinations(bk):
  enc, dec, in_shape, _ = tiny_spec()
  mk = lambda **kw: VAEEngine(enc, dec, in_shape, kw.pop('zdim', 5), 4, bk.dev, lib=bk.L,
                              latent_dist=kw.pop('latent_dist', 'relaxedonehot'), **kw)
  other = VAEEngine(enc, dec, in_shape, 5, 4, bk.dev, lib=bk.L)
  for kw, exc, word in ((dict(tc='betatc'), ValueError, 'tc'), (dict(latent_reg='mmd'), ValueError, 'mmd'),
                        (dict(latent_reg='dip_i'), ValueError, 'dip_i'), (dict(latent_reg='dip_ii'), ValueError, 'dip_ii'),
                        (dict(vamprior_components=3), ValueError, 'vamprior'),
                        (dict(vq_codes=5), ValueError, 'vq_codes'),
                        (dict(latent_cov='tril'), ValueError, 'tril'),
                        (dict(zdim=1), ValueError, 'zdim'), (dict(zdim=65), ValueError, 'zdim'),
                        (dict(temperature=0.0), ValueError, 'temperature'),
                        (dict(neck_bwd=True), NotImplementedError, 'neck_bwd'),
                        (dict(world_size=2), NotImplementedError, 'data parallel'),
                        (dict(force_dp=True), NotImplementedError, 'data parallel'),
                        (dict(range_words=other.range_words), NotImplementedError, 'range_words'),
                        (dict(analytic=True, reverse=False), NotImplementedError, 'reverse'),
                        (dict(latent_dist='bernoulli'), ValueError, 'latent_dist')):
    with pytest.raises(exc, match=word):
      mk(**kw)
  with pytest.raises(ValueError, match='latent_cov'):   # (as before)
    VAEEngine(enc, dec, in_shape, 5, 4, bk.dev, lib=bk.L, latent_cov='full')
  eng = mk(temperature=0.7)
  assert eng.temperature == 0.7 and eng.latent_dist == 'relaxedonehot'
  with pytest.raises(NotImplementedError, match='reverse'):
    eng.set_kl_form(True, reverse=False)


def test_fused_forms_are_ignored_and_no_rng_launch(bk):
  spec = neck_spec(5, 128)
  assert VAEEngine(*spec, 2, bk.dev, lib=bk.L, neck=True).neck
  calls = []
  eng = VAEEngine(*spec, 2, bk.dev, lib=Recorder(bk.L, calls), neck=True, latent_dist='relaxedonehot')
  assert not (eng.neck or eng.lat_block) and eng.pw == 5
  x, _ = case_data(bk.dev, spec, B=2)
  calls.clear()
  eng.train_step(x, None, lr=1e-3, beta=2.0)   # (forward(fused=True): the default; the noise is drawn in the kernel)
  assert not [c for c in calls if 'neck' in c or 'latent_block' in c or 'odin_rng_' in c
              or c in ('odin_latent_fwd', 'odin_latent_bwd')]
  assert calls.count('odin_latent_concrete_fwd') == 1 and calls.count('odin_latent_concrete_bwd') == 1
  i = calls.index('odin_latent_concrete_fwd')
  assert calls[i - 1] == 'odin_dense_fwd'
  j = calls.index('odin_latent_concrete_bwd')
  assert i < j and calls[j + 1:j + 3] == ['odin_dense_wgrad', 'odin_dense_bwd']
  assert bool(torch.isfinite(eng.out4).all()) and bool(torch.isfinite(eng.eps).all())
  assert torch.allclose(eng.z.sum(1), torch.ones(2, device=eng.z.device), rtol=0, atol=1e-5)
  # the noise the step left behind is the stream of (seed, step)
  assert eng.step_count == 1 and np.array_equal(eng.eps.cpu().numpy().ravel(), rng_gumbel(bk, 10, eng.seed, 1))


def test_plain_engine_call_list_is_unchanged(bk):
  eng, c1 = launch_record(bk)
  assert c1 == PLAIN_STEP_CALLS and eng.latent_dist == 'normal' and eng.pw == 2 * eng.D
  _, c2 = launch_record(bk, latent_dist='normal', temperature=0.5)
  assert c2 == PLAIN_STEP_CALLS
  nl = len(eng.enc_recs) + len(eng.dec_recs)
  assert eng.range_words.numel() == 2 * nl * RANGE_WORDS


# ---- 6. the model API ---------------------------------------------------------------------------------------------------
def concrete_nets(K=5, C=1, alias='relaxedonehot', **kwargs):
  from odin_ai_amd.networks import RVconf
  nets = tiny_nets(C=C, zdim=K)
  nets['latents'] = RVconf(K, alias, projection=True, name='latents', kwargs=dict(kwargs))
  return nets


def api_x(B=6, seed=2):
  return np.clip(np.random.default_rng(seed).random((B, 8, 8, 1)), 1e-6, 1 - 1e-6).astype(np.float32)


def test_api_quick_start_builds_fits_and_returns_the_posterior(bk):
  from odin_ai_amd.vae import BetaVAE, RelaxedOneHotPosterior
  K, tau = 5, 0.7
  vae = BetaVAE(beta=2.0, device=bk.dev, lib=bk.L, **concrete_nets(K, alias='relaxedsoftmax', temperature=tau))
  x = api_x(8)
  before, _ = vae.optimize(x, training=False)
  vae.fit(x, max_iter=3, batch_size=8, learning_rate=1e-3, compile_graph=False)
  assert vae.step == 3 and np.isfinite(float(vae.optimize(x, training=False)[0])) and np.isfinite(float(before))
  g = np.random.default_rng(1).gumbel(size=(8, K)).astype(np.float32)
  px, qz = vae(x, eps=g)
  assert isinstance(qz, RelaxedOneHotPosterior) and qz.event_shape == (K,) and qz.batch_shape == (8,)
  assert qz.temperature == tau and qz.logits.shape == (8, K)
  assert torch.allclose(qz.probs.sum(-1), torch.ones(8, device=qz.logits.device), rtol=0, atol=1e-6)
  with pytest.raises(NotImplementedError):
    qz.mean()
  s = qz.sample(3, seed=1)
  assert s.shape == (3, 8, K) and torch.equal(s, qz.sample(3, seed=1)) and bool((s >= 0).all())
  assert torch.allclose(s.sum(-1), torch.ones(3, 8, device=s.device), rtol=0, atol=1e-5)
  # the posterior's own numbers against the restatement (the logits as the engine left them)
  l64, g64 = cu.t64(qz.logits.cpu().numpy()), cu.t64(g)
  y64, z64 = cu.relax(l64, g64, tau)
  z = qz.tensor()
  close(z.cpu().numpy(), z64.numpy())
  close(qz.log_prob(z).cpu().numpy(), cu.log_q(l64, y64, tau).numpy())
  close(qz.KL_divergence(analytic=True).cpu().numpy(), cu.kl_categorical(l64).numpy())
  close(qz.KL_divergence(analytic=False).cpu().numpy(), cu.kl_mc(l64, g64, tau).numpy())
  fb = qz.KL_divergence(analytic=True, free_bits=0.4, keepdims=True)
  assert fb.shape == (1, 8) and float(fb.min()) >= 0.4 * K - 1e-6
  with pytest.raises(NotImplementedError, match='reverse'):
    qz.KL_divergence(analytic=True, reverse=False)
  # elbo_components: the engine's KL (times beta) is the wrapper's KL at the engine's sample
  llk, kl = vae.elbo_components(x, eps=g)
  _, q2 = vae.last_outputs
  assert llk['llk_image'].shape == (8,) and kl['kl_latents'].shape == (8,)
  close(kl['kl_latents'].cpu().numpy(), 2.0 * q2.KL_divergence(analytic=False).cpu().numpy())
  assert np.isfinite(vae.elbo(llk, kl).cpu().numpy()).all()
  assert vae.trainable_variables[('lat', 'w')].shape == (24, K) and vae.variable_name(('lat', 'w')) == 'latents/kernel'
  # the prior's samples: one-hot rows, seeded
  zp = vae.sample_prior(4, seed=3)
  assert zp.shape == (4, K) and bool(((zp == 0) | (zp == 1)).all()) and bool((zp.sum(1) == 1).all())
  assert torch.equal(zp, vae.sample_prior(4, seed=3))
  assert vae.decode(zp, only_decoding=True).shape == (4, 8, 8, 1)


def test_marginal_log_prob_matches_float64_logmeanexp(bk):
  from odin_ai_amd.vae import VariationalAutoencoder
  from oracle.torch_ref import TorchVAE, t_seq
  K, n, N, tau = 5, 3, 6, 0.5
  vae = VariationalAutoencoder(device=bk.dev, lib=bk.L, **concrete_nets(K))
  x = api_x(N)
  g = np.random.default_rng(4).gumbel(size=(n, N, K)).astype(np.float32)
  llk, lat = vae.marginal_log_prob(x, n_mcmc=n, reduce=None, batch_size=4, eps=g)
  T = {k: torch.as_tensor(v.cpu().numpy(), dtype=F64) for k, v in vae.trainable_variables.items()}
  x64 = torch.as_tensor(x, dtype=F64)
  h_e = t_seq(vae.encoder.layers, TorchVAE._sub(T, 'enc'), x64)
  l64 = (h_e @ T[('lat', 'w')] + T[('lat', 'b')])[None].expand(n, N, K)
  y64, z64 = cu.relax(l64, cu.t64(g), tau)
  h_d = t_seq(vae.decoder.layers, TorchVAE._sub(T, 'dec'), z64.reshape(n * N, K)).reshape((n, N, 8, 8, 1))
  lme = lambda t: (torch.logsumexp(t, 0) - math.log(n)).numpy()
  close(llk['image'].cpu().numpy(), lme((x64[None] * h_d - cu.softplus(h_d)).reshape(n, N, -1).sum(-1)))
  close(lat['latents'][0].cpu().numpy(), lme(cu.log_q(l64, y64, tau)))
  close(lat['latents'][1].cpu().numpy(), lme(cu.log_p(z64)))
  # without explicit noise: drawn on the device, finite
  llk2, lat2 = vae.marginal_log_prob(x, n_mcmc=n, reduce=None, batch_size=4)
  assert all(bool(torch.isfinite(t).all()) for t in (llk2['image'],) + tuple(lat2['latents']))


@pytest.mark.parametrize('fmt', ['npz', 'tf'])
def test_api_save_load_round_trip(bk, tmp_path, fmt):
  from odin_ai_amd.vae import BetaVAE
  vae = BetaVAE(beta=2.0, device=bk.dev, lib=bk.L, **concrete_nets(5))
  x = api_x()
  vae.optimize(x, learning_rate=1e-2)
  path = str(tmp_path / 'w')
  vae.save_weights(path, save_format=fmt)
  other = BetaVAE(beta=2.0, device=bk.dev, lib=bk.L, seed=3, **concrete_nets(5))
  assert not torch.equal(other.trainable_variables[('lat', 'w')], vae.trainable_variables[('lat', 'w')])
  other.load_weights(path, raise_notfound=True)
  assert other.step == 1
  for k, v in vae.trainable_variables.items():
    assert torch.equal(v, other.trainable_variables[k]), k
  g = np.random.default_rng(1).gumbel(size=(6, 5)).astype(np.float32)
  a, b = vae.elbo_components(x, eps=g), other.elbo_components(x, eps=g)
  assert torch.equal(a[0]['llk_image'], b[0]['llk_image']) and torch.equal(a[1]['kl_latents'], b[1]['kl_latents'])


def test_api_supported_and_refused_classes(bk):
  from odin_ai_amd.networks import get_networks
  from odin_ai_amd.vae import get_vae
  x = api_x()
  for name, kw in (('vae', {}), ('betavae', dict(beta=2.0)), ('annealingvae', {}), ('betacapacityvae', {})):
    vae = get_vae(name)(device=bk.dev, lib=bk.L, **kw, **concrete_nets(5))
    vae.fit(x, max_iter=2, batch_size=6, learning_rate=1e-3, compile_graph=False)
    eng = vae._engine(6)
    assert vae.step == 2 and eng.latent_dist == 'relaxedonehot' and eng.temperature == 0.5, name
    llk, kl = vae.elbo_components(x)
    assert llk['llk_image'].shape == (6,) and kl['kl_latents'].shape == (6,), name
    assert bool(torch.isfinite(llk['llk_image']).all()) and bool(torch.isfinite(kl['kl_latents']).all()), name
  for name in ('betatcvae', 'infovae', 'dipvae', 'vampriorvae', 'vqvae', 'factorvae'):
    with pytest.raises(ValueError, match='relaxedonehot'):
      get_vae(name)(device=bk.dev, lib=bk.L, **concrete_nets(5))
  vae = get_vae('vae')(device=bk.dev, lib=bk.L, analytic=True, free_bits=0.3, sample_shape=(2,), **concrete_nets(5))
  llk, kl = vae.elbo_components(x)
  assert llk['llk_image'].shape == (2, 6) and kl['kl_latents'].shape == (1, 6)
  assert float(kl['kl_latents'].min()) >= 0.3 * 5 - 1e-6
  assert np.isfinite(float(vae.optimize(x, learning_rate=1e-3)[0]))
  # reverse=False: at construction, in set_elbo_configs and in the engine's set_kl_form
  with pytest.raises(NotImplementedError, match='reverse'):
    vae.set_elbo_configs(reverse=False)
  with pytest.raises(NotImplementedError, match='reverse'):
    get_vae('vae')(device=bk.dev, lib=bk.L, analytic=True, reverse=False, **concrete_nets(5))
  with pytest.raises(NotImplementedError, match='reverse'):
    vae._engine(6).set_kl_form(True, reverse=False)
  with pytest.raises(ValueError, match='temperature'):
    get_vae('vae')(device=bk.dev, lib=bk.L, **concrete_nets(5, temperature=0.0))
  assert get_networks('dsprites', qz='relaxedonehot')['latents'].posterior == 'relaxedonehot'
