"""The relaxed Bernoulli (binary Concrete) posterior 'relaxedbernoulli' (latent_binconcrete.hip,
VAEEngine(latent_dist='relaxedbernoulli'), RelaxedBernoulliPosterior) on both backends of the `bk` fixture: the float64
restatement of tests/relaxedbern_util.py against torch's own LogitRelaxedBernoulli / RelaxedBernoulli / Bernoulli and
autograd, the logistic stream, the kernels against that restatement, whole training steps against float64 autograd, the
engine's behaviour and the model API.

Tolerances (the project's own, tests/test_latent_concrete.py): 1e-4 of a tensor's maximum for values and gradients; the
restatement against torch.distributions to 1e-9; fbmask and everything the kernels promise bit for bit, exactly.

torch's RelaxedBernoulli.log_prob(z) takes logit(z) and is off by up to 2.5 at tau = 0.1: the restatement is compared
with the logit-space density LogitRelaxedBernoulli.log_prob(u) plus the Jacobian of the sigmoid everywhere, and with
RelaxedBernoulli.log_prob(z) only at tau in {0.5, 1} with logits in [-1, 1] and U in [0.05, 0.95].

Free bits "clamp some but not all samples": the threshold (and the capacity) lies in the middle of the (second) widest
gap between two KL values of the drawn batch, as tests/test_latent_tril.py places it (asserted: both kinds occur, and no
sample sits within twice the parity bound of a threshold).  A batch of ONE sample cannot hold both kinds: there the
kernel runs once under a threshold above the sample's KL and once under one below it.

The logistic stream's moments over n = 200 001: mean within 0.0203 of 0, variance within 0.066 of pi^2 / 3 -- five
standard errors of either estimate at this n (sigma = pi / sqrt(3): sd of the mean 0.00406; of the variance
sigma^2 sqrt(3.2 / n) = 0.0132 with the logistic's mu4 = 4.2 sigma^4).

Whole steps: the loss and the projection's gradient at the parity bound; every element of every parameter after three
Adam steps to 2e-4 of its tensor's largest weight, the bar of the other models' step tests (tests/test_vq.py)."""
import math

import numpy as np
import pytest
import torch

from odin_ai_amd._lib import OdinError
from odin_ai_amd.engine import RANGE_WORDS, VAEEngine
from oracle import vae_oracle as vo
from tests import relaxedbern_util as ru
from tests.engine_util import Recorder, case_data, launch_record, neck_spec, tiny_nets, tiny_spec
from tests.test_latent_regularizers import _adam_ref
from tests.test_vamprior import PLAIN_STEP_CALLS

F64 = torch.float64
TAUS = [0.1, 0.5, 1.0]


def close(got, ref, tol=1e-4):
  got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
  scale = max(float(np.abs(ref).max()), 1e-30)
  err = float(np.abs(got - ref).max())
  assert err <= tol * scale, (err, scale)


def sync(bk):
  if bk.dev.type == 'cuda':
    torch.cuda.synchronize()


# ---- 1. the restatement against torch's own distributions --------------------------------------------------------------
def _draw64(B, D, seed, std=3.0):
  gen = torch.Generator().manual_seed(seed)
  l = torch.randn(B, D, generator=gen, dtype=F64) * std
  U = torch.rand(B, D, generator=gen, dtype=F64).clamp(1e-12, 1 - 1e-12)
  return l, ru.logistic_of(U)


@pytest.mark.parametrize('tau', TAUS)
@pytest.mark.parametrize('D', [1, 2, 10, 64, 200])
def test_restatement_matches_torch_distributions(D, tau):
  from torch.distributions import Bernoulli, RelaxedBernoulli, kl_divergence
  from torch.distributions.relaxed_bernoulli import LogitRelaxedBernoulli
  B = 6
  tol = dict(rtol=0, atol=1e-9)
  l, n = _draw64(B, D, 10 + D)
  u, z = ru.relax(l, n, tau)
  t = torch.tensor(tau, dtype=F64)
  ref = LogitRelaxedBernoulli(t, logits=l).log_prob(u).sum(-1)
  assert torch.allclose(ru.log_q_logit(l, u, tau), ref, **tol)
  assert torch.allclose(ru.log_q(l, u, tau), ref + (ru.softplus(u) + ru.softplus(-u)).sum(-1), **tol)
  assert torch.allclose(ru.kl_mc(l, n, tau), ru.log_q(l, u, tau) + D * math.log(2.0), **tol)
  # the prior on the closed cube, corners included, and the closed-form KL
  prior = Bernoulli(logits=torch.zeros(B, D, dtype=F64))
  corners = (z > 0.5).to(F64)
  assert torch.allclose(ru.log_p(z), prior.log_prob(corners).sum(-1), **tol)
  assert torch.allclose(ru.kl_bernoulli(l), kl_divergence(Bernoulli(logits=l), prior).sum(-1), **tol)
  if tau >= 0.5:   # torch's own density on the cube, where its logit(z) is still accurate
    gen = torch.Generator().manual_seed(30 + D)
    l2 = torch.rand(B, D, generator=gen, dtype=F64) * 2.0 - 1.0
    n2 = ru.logistic_of(0.05 + 0.9 * torch.rand(B, D, generator=gen, dtype=F64))
    u2, z2 = ru.relax(l2, n2, tau)
    assert torch.allclose(ru.log_q(l2, u2, tau), RelaxedBernoulli(t, logits=l2).log_prob(z2).sum(-1), **tol)


@pytest.mark.parametrize('analytic', [False, True])
@pytest.mark.parametrize('tau', TAUS)
@pytest.mark.parametrize('D', [1, 2, 10, 64, 200])
def test_hand_gradients_match_autograd(D, tau, analytic):
  B = 5
  l, n = _draw64(B, D, 20 + D)
  G = torch.randn(B, D, dtype=F64, generator=torch.Generator().manual_seed(3))
  fb = torch.tensor([1.0, 0.0, 1.0, -1.0, 1.0], dtype=F64)   # (clamped | capacity's sign among them)
  klw = 0.37
  lt = l.clone().requires_grad_(True)
  kl = ru.kl_bernoulli(lt) if analytic else ru.kl_mc(lt, n, tau)
  ((klw * fb * kl).sum() + (G * ru.relax(lt, n, tau)[1]).sum()).backward()
  hand = ru.latent_bwd(l, n, G, fb, klw, tau, analytic)
  assert float((hand - lt.grad).abs().max()) <= 1e-9 * max(1.0, float(lt.grad.abs().max()))


# ---- 2. the logistic stream ---------------------------------------------------------------------------------------------
def rng_logistic(bk, n, seed, step=None):
  out = bk.full((n,), float('nan'))
  st = bk.T(np.array([step]), torch.int32) if step is not None else None
  bk.L.odin_rng_logistic(out.data_ptr(), n, seed, st.data_ptr() if st is not None else None, None)
  sync(bk)
  return out.cpu().numpy()


def test_rng_logistic_stream(bk):
  n = 200001
  a, b, c = rng_logistic(bk, n, 11, 4), rng_logistic(bk, n, 11, 4), rng_logistic(bk, n, 11, 5)
  assert np.array_equal(a, b) and not np.array_equal(a, c)
  assert np.array_equal(rng_logistic(bk, n, 11), rng_logistic(bk, n, 11, 0))   # (no step word: step 0)
  assert np.isfinite(a).all() and np.abs(a).max() <= 17.33
  a64 = a.astype(np.float64)
  print(f'logistic stream: mean = {a64.mean():+.5f}, var - pi^2/3 = {a64.var() - math.pi ** 2 / 3:+.5f}, '
        f'range [{a64.min():.3f}, {a64.max():.3f}]')
  assert abs(a64.mean()) <= 0.0203
  assert abs(a64.var() - math.pi ** 2 / 3) <= 0.066


def run_fwd(bk, p, n, tau, analytic, free_bits=None, capacity=None, draw=None):
  """draw: None (the noise n is read) | (seed, step): drawn in the kernel; -> z, kl, fbmask, the noise buffer"""
  B, D = p.shape
  z, kl, m = bk.full((B, D), float('nan')), bk.full((B,), float('nan')), bk.full((B,), float('nan'))
  pt = bk.T(p)
  nt = bk.T(n) if draw is None else bk.full((B, D), float('nan'))
  cap = bk.T(np.array([capacity], np.float32)) if capacity is not None else None
  st = bk.T(np.array([draw[1]]), torch.int32) if draw is not None else None
  bk.L.odin_latent_relaxedbern_fwd(pt.data_ptr(), nt.data_ptr(), z.data_ptr(), kl.data_ptr(), m.data_ptr(), B, D,
                                   float(tau), int(analytic), -1.0 if free_bits is None else float(free_bits),
                                   cap.data_ptr() if cap is not None else None, int(draw is not None),
                                   draw[0] if draw is not None else 0, st.data_ptr() if st is not None else None, None)
  sync(bk)
  return z.cpu().numpy(), kl.cpu().numpy(), m.cpu().numpy(), nt.cpu().numpy()


@pytest.mark.parametrize('B,D', [(6, 10), (5, 3)])   # (15 elements: no multiple of the counter's 4)
def test_forward_draws_the_logistic_stream_bit_for_bit(bk, B, D):
  p = (np.random.default_rng(B).standard_normal((B, D)) * 1.5).astype(np.float32)
  stream = rng_logistic(bk, B * D, 2 ** 33 + 5, 9).reshape(B, D)
  z, kl, m, n = run_fwd(bk, p, None, 0.5, 0, draw=(2 ** 33 + 5, 9))
  assert np.array_equal(n, stream)
  # and the sample is the one the explicit noise gives
  z2, kl2, m2, _ = run_fwd(bk, p, stream, 0.5, 0)
  assert np.array_equal(z, z2) and np.array_equal(kl, kl2) and np.array_equal(m, m2)
  close(z, ru.latent_fwd(p, stream, 0.5, 0)[0].numpy())


# ---- 3. the kernels against float64 -------------------------------------------------------------------------------------
# a lone unit and a lone sample | a partial last workgroup | more than one workgroup | the lane stride (64), its first
# second round (65), a partial fourth round (200) and the widest one (255)
KERNEL_SIZES = [(1, 1), (1, 2), (5, 3), (6, 10), (3, 64), (3, 65), (2, 200), (2, 255)]


def draw32(B, D, seed, std=1.5):
  """float32 (logits, logistic noise)"""
  rng = np.random.default_rng(seed)
  return (rng.standard_normal((B, D)) * std).astype(np.float32), rng.logistic(size=(B, D)).astype(np.float32)


def run_bwd(bk, p, n, z, dz, dzx, m, klw, tau, analytic):
  B, D = p.shape
  dp = bk.full(p.shape, float('nan'))
  ts = [bk.T(a) if a is not None else None for a in (p, n, z, dz, dzx, m, np.array([klw], np.float32))]
  a = [t.data_ptr() if t is not None else None for t in ts]
  bk.L.odin_latent_relaxedbern_bwd(a[0], a[1], a[2], a[3], a[4], a[5], a[6], dp.data_ptr(), B, D, float(tau),
                                   int(analytic), None)
  sync(bk)
  return dp.cpu().numpy()


def thresholds(raw_kl, D):
  """-> [(free_bits, capacity)] for the case, from the float64 KL of the drawn batch: the free-bits threshold in the
  middle of the widest gap between two consecutive KL values, the capacity in the middle of the second widest (two
  samples: at three quarters of the one gap); ONE sample: a threshold above its KL, then one below it"""
  s = np.sort(raw_kl)
  if len(s) == 1:
    assert s[0] > 0.2, 'the single sample needs a KL a positive threshold fits under'
    return [(float(np.float32((s[0] + 1.0) / D)), float(np.float32(s[0] - 0.7))),
            (float(np.float32(s[0] / (2 * D))), float(np.float32(s[0] + 0.7)))]
  order = np.argsort(np.diff(s))[::-1]
  k = order[0]
  fb = float(np.float32(0.5 * (s[k] + s[k + 1]) / D))
  c = 0.25 * s[0] + 0.75 * s[1] if len(s) == 2 else 0.5 * (s[order[1]] + s[order[1] + 1])
  return [(fb, float(np.float32(c)))]


def check_case(bk, p, n, tau, analytic, clamps=True):
  """forward and backward of one drawn batch against float64: without and with free bits / a capacity, with either
  incoming gradient absent"""
  B, D = p.shape
  rng = np.random.default_rng(B + D)
  dz = (rng.standard_normal((B, D)) * 0.3).astype(np.float32)
  dzx = (rng.standard_normal((B, D)) * 0.2).astype(np.float32)
  klw = float(np.float32(1.5 / B))
  raw = ru.latent_fwd(p, n, tau, analytic)[3].numpy()
  cases = [(None, None)]
  if clamps:
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
    cases += [(f, None) for f, _ in ths] + [(None, c) for _, c in ths] + ths
  for fb, cap in cases:
    z64, kl64, m64, _ = ru.latent_fwd(p, n, tau, analytic, fb, cap)
    z, kl, m, _ = run_fwd(bk, p, n, tau, analytic, fb, cap)
    assert np.isfinite(z).all() and np.isfinite(kl).all()   # (every element written: the buffers started as NaN)
    close(z, z64.numpy())
    close(kl, kl64.numpy())
    assert np.array_equal(m, m64.numpy().astype(np.float32)), (fb, cap, m, m64)
    for a, b in ((dz, dzx), (dz, None), (None, dzx), (None, None)):
      G = sum(v.astype(np.float64) for v in (a, b) if v is not None) if (a is not None or b is not None) \
          else np.zeros((B, D))
      ref = ru.latent_bwd(p, n, G, m64.numpy(), klw, tau, analytic).numpy()
      dp = run_bwd(bk, p, n, z, a, b, m, klw, tau, analytic)
      assert np.isfinite(dp).all()
      if np.abs(ref).max() == 0.0:   # (B = 1 under free bits without an incoming gradient: every term vanishes)
        assert not dp.any()
      else:
        close(dp, ref)
  return z, m


@pytest.mark.parametrize('analytic', [0, 1])
@pytest.mark.parametrize('tau', TAUS)
@pytest.mark.parametrize('B,D', KERNEL_SIZES)
def test_kernels_match_float64(bk, B, D, tau, analytic):
  # (B = 1: the seed is one whose single-sample KL leaves room for a positive threshold under it -- asserted)
  seed = 3 if B == 1 else 100 * B + D
  p, n = draw32(B, D, seed)
  z, m = check_case(bk, p, n, tau, analytic)
  # the stored z is not read by the backward (its gradients are formed in u): it may be absent
  klw = 0.25
  dz = np.ones((B, D), np.float32)
  assert np.array_equal(run_bwd(bk, p, n, None, dz, None, m, klw, tau, analytic),
                        run_bwd(bk, p, n, z, dz, None, m, klw, tau, analytic))


@pytest.mark.parametrize('B,D', [(1, 1), (6, 10), (3, 65), (2, 255)])
def test_closed_form_kl_near_zero_logits(bk, B, D):
  """logits of a freshly initialised projection (x 0.01): the Bernoulli KL is about l^2 / 8 per unit, 1e-5 and below,
  formed from terms near log 2 in its textbook form -- the bound is taken on that tensor's own tiny maximum"""
  p, n = draw32(B, D, 7 * B + D, std=0.01)
  raw = ru.latent_fwd(p, n, 0.5, 1)[3].numpy()
  assert 0 < raw.max() < 1e-4 * D
  z, kl, m, _ = run_fwd(bk, p, n, 0.5, 1)
  close(kl, raw)
  close(z, ru.latent_fwd(p, n, 0.5, 1)[0].numpy())
  dp = run_bwd(bk, p, n, z, None, None, m, 0.75, 0.5, 1)   # (the KL's gradient alone: w l / 4, tiny as well)
  close(dp, ru.latent_bwd(p, n, np.zeros((B, D)), m, 0.75, 0.5, 1).numpy())


def run_sample_logprob(bk, p, n, tau):
  ns, B, D = n.shape
  z, lq, lp = bk.full((ns, B, D), float('nan')), bk.full((ns, B), float('nan')), bk.full((ns, B), float('nan'))
  pt, nt = bk.T(p), bk.T(n)
  bk.L.odin_latent_relaxedbern_sample_logprob(pt.data_ptr(), nt.data_ptr(), z.data_ptr(), lq.data_ptr(), lp.data_ptr(), ns,
                                              B, D, float(tau), None)
  sync(bk)
  return z.cpu().numpy(), lq.cpu().numpy(), lp.cpu().numpy()


def test_low_temperature_saturation_stays_finite(bk):
  """tau = 0.1, logits of standard deviation 4: |u| passes 104, z rounds to exactly 0 and exactly 1 in float32, and
  everything that is computed in u stays finite and at the parity bound"""
  tau, B, D = 0.1, 16, 10
  p, n = draw32(B, D, 3, std=4.0)
  u64, z64 = ru.relax(ru.t64(p), ru.t64(n), tau)
  assert float(u64.min()) < -110.0 and float(u64.max()) > 20.0
  for analytic in (0, 1):
    z, kl, m, _ = run_fwd(bk, p, n, tau, analytic)
    assert (z == 0.0).any() and (z == 1.0).any() and np.isfinite(z).all() and np.isfinite(kl).all()
    _, kl64, m64, _ = ru.latent_fwd(p, n, tau, analytic)
    close(z, z64.numpy())
    close(kl, kl64.numpy())
    rng = np.random.default_rng(1)
    dz = (rng.standard_normal((B, D)) * 0.3).astype(np.float32)
    dp = run_bwd(bk, p, n, z, dz, None, m, 0.25, tau, analytic)
    assert np.isfinite(dp).all()
    close(dp, ru.latent_bwd(p, n, dz, m64.numpy(), 0.25, tau, analytic).numpy())
  zs, lq, lp = run_sample_logprob(bk, p, n[None], tau)
  assert np.isfinite(lq).all() and np.array_equal(zs[0], z)
  close(lq[0], ru.log_q(ru.t64(p), u64, tau).numpy())
  close(lp[0], ru.log_p(z64).numpy())


@pytest.mark.parametrize('B,D,tau', [(5, 3, 0.5), (3, 65, 1.0), (6, 10, 0.1), (1, 1, 0.5), (2, 255, 0.5)])
def test_sample_logprob_matches_float64(bk, B, D, tau):
  ns = 3
  p, _ = draw32(B, D, 7 * B + D)
  n = np.random.default_rng(ns).logistic(size=(ns, B, D)).astype(np.float32)
  z, lq, lp = run_sample_logprob(bk, p, n, tau)
  l64, n64 = ru.t64(p)[None].expand(ns, B, D), ru.t64(n)
  u64, z64 = ru.relax(l64, n64, tau)
  close(z, z64.numpy())
  close(lq, ru.log_q(l64, u64, tau).numpy())
  close(lp, ru.log_p(z64).numpy())


def test_kernels_are_bit_reproducible(bk):
  p, n = draw32(9, 130, 5)
  a, b = run_fwd(bk, p, n, 0.5, 0), run_fwd(bk, p, n, 0.5, 0)
  assert all(np.array_equal(x, y) for x, y in zip(a, b))
  dz = np.ones((9, 130), np.float32)
  r1 = run_bwd(bk, p, n, a[0], dz, None, a[2], 0.1, 0.5, 0)
  r2 = run_bwd(bk, p, n, a[0], dz, None, a[2], 0.1, 0.5, 0)
  assert np.array_equal(r1, r2)


def test_out_of_range_arguments_return_the_error_code(bk):
  B = 2
  p, n = bk.zeros(B, 256), bk.zeros(3 * B, 256)
  outs = [bk.full((3 * B, 256), 7.0), bk.full((B,), 7.0), bk.full((B,), 7.0), bk.full((B, 256), 7.0),
          bk.full((3 * B,), 7.0)]
  z, kl, m, dp, lq = outs
  one = bk.full((1,), 1.0)
  for D, tau, analytic, word in ((0, 0.5, 0, 'D outside'), (256, 0.5, 0, 'D outside'), (4, 0.0, 0, 'temperature'),
                                 (4, -1.0, 0, 'temperature'), (4, 0.5, 2, 'analytic')):
    for draw in (0, 1):
      with pytest.raises(OdinError, match=word) as e:
        bk.L.odin_latent_relaxedbern_fwd(p.data_ptr(), n.data_ptr(), z.data_ptr(), kl.data_ptr(), m.data_ptr(), B, D, tau,
                                         analytic, -1.0, None, draw, 1, None, None)
      assert 'rc=-2' in str(e.value)
    with pytest.raises(OdinError, match=word) as e:
      bk.L.odin_latent_relaxedbern_bwd(p.data_ptr(), n.data_ptr(), z.data_ptr(), z.data_ptr(), None, m.data_ptr(),
                                       one.data_ptr(), dp.data_ptr(), B, D, tau, analytic, None)
    assert 'rc=-2' in str(e.value)
    if analytic == 0:
      with pytest.raises(OdinError, match=word) as e:
        bk.L.odin_latent_relaxedbern_sample_logprob(p.data_ptr(), n.data_ptr(), z.data_ptr(), lq.data_ptr(),
                                                    lq.data_ptr(), 3, B, D, tau, None)
      assert 'rc=-2' in str(e.value)
  for draw in (0, 1):
    with pytest.raises(OdinError, match='batch') as e:
      bk.L.odin_latent_relaxedbern_fwd(p.data_ptr(), n.data_ptr(), z.data_ptr(), kl.data_ptr(), m.data_ptr(), 0, 4, 0.5, 0,
                                       -1.0, None, draw, 1, None, None)
    assert 'rc=-2' in str(e.value)
  with pytest.raises(OdinError, match='batch'):
    bk.L.odin_latent_relaxedbern_bwd(p.data_ptr(), n.data_ptr(), z.data_ptr(), z.data_ptr(), None, m.data_ptr(),
                                     one.data_ptr(), dp.data_ptr(), 0, 4, 0.5, 0, None)
  with pytest.raises(OdinError, match='positive'):
    bk.L.odin_latent_relaxedbern_sample_logprob(p.data_ptr(), n.data_ptr(), z.data_ptr(), lq.data_ptr(), lq.data_ptr(), 3,
                                                0, 4, 0.5, None)
  sync(bk)
  assert all(bool((t == 7.0).all()) for t in outs) and bool((n == 0.0).all())


# ---- 4. whole training steps against float64 autograd -------------------------------------------------------------------
def relaxedbern_case(bk, spec, B, seed=7, **engkw):
  """-> engine (latent_dist='relaxedbernoulli'), its parameters as float64 arrays (the networks' through OracleVAE's
  initialiser, the projection drawn here: its shape is the new one), x, the logistic noise"""
  enc, dec, in_shape, D = spec
  eng = VAEEngine(enc, dec, in_shape, D, B, bk.dev, lib=bk.L, latent_dist='relaxedbernoulli', **engkw)
  rng = np.random.default_rng(seed)
  P = vo.OracleVAE(enc, dec, in_shape, D, observation='bernoulli').init_params(seed=5)
  P = {k: np.asarray(v, np.float64) for k, v in P.items() if k[0] != 'lat'}
  P[('lat', 'w')] = (rng.standard_normal((eng.hdim, D)) * 0.3).astype(np.float32).astype(np.float64)
  P[('lat', 'b')] = (rng.standard_normal(D) * 0.1).astype(np.float32).astype(np.float64)
  eng.load_params(P)
  x = np.clip(rng.random((B,) + tuple(in_shape)), 1e-6, 1 - 1e-6).astype(np.float32)
  return eng, P, x, rng.logistic(size=(B, D)).astype(np.float32)


STEP_KL = [('mc', False, 1.5), ('analytic', True, 0.4)]
STEP_CASES = [(f'{sid}_D{D}_{cid}{"_free_bits" if fb else ""}', sid, D, analytic, beta, fb)
              for sid, D in (('tiny', 5), ('tiny', 70)) for cid, analytic, beta in STEP_KL for fb in (False, True)]


@pytest.mark.parametrize('name,sid,D,analytic,beta,fb', STEP_CASES, ids=[c[0] for c in STEP_CASES])
def test_three_train_steps_follow_float64_adam(bk, name, sid, D, analytic, beta, fb):
  spec, B, lr = tiny_spec(D), 6, 1e-3
  free_bits = None
  if fb:
    # the threshold in the widest gap of the batch's KL values at the first step (float64, no free bits)
    eng, P, x, n = relaxedbern_case(bk, spec, B, hyper_ring_rows=16, analytic=analytic)
    f0 = ru.RelaxedBernRef(spec[0], spec[1], D, 0.5, analytic, beta).loss_and_grads(P, x, n)[0]
    s = np.sort(f0['kl'])
    k = int(np.argmax(np.diff(s)))
    free_bits = float(np.float32(0.5 * (s[k] + s[k + 1]) / D))
    assert free_bits > 0, s
  eng, P, x, n = relaxedbern_case(bk, spec, B, hyper_ring_rows=16, analytic=analytic, free_bits=free_bits)
  assert eng.p.shape == (B, D) and eng.dp.shape == (B, D) and eng.eps.shape == (B, D) and not (eng.lat_block or eng.neck)
  ref = ru.RelaxedBernRef(spec[0], spec[1], D, 0.5, analytic, beta, free_bits)
  M = {k: np.zeros_like(v) for k, v in P.items()}
  V = {k: np.zeros_like(v) for k, v in P.items()}
  xt, nt = bk.T(x), bk.T(n)
  for t in (1, 2, 3):
    f, G, dp = ref.loss_and_grads(P, x, n)
    if t == 1 and fb:
      hit = f['kl'] <= free_bits * D + 1e-12
      assert hit.any() and not hit.all(), f['kl']
    out = eng.train_step(xt, nt, lr=lr, beta=beta).cpu().numpy()
    assert abs(out[0] - f['loss']) <= 1e-4 * max(1.0, abs(f['loss'])), (t, out[0], f['loss'])
    close(eng.kl.cpu().numpy(), f['kl'])
    close(eng.dp.cpu().numpy(), dp)   # the projection's gradient: of its output, its kernel and its bias
    gv = {k: v.cpu().numpy() for k, v in eng.grad_views().items()}
    assert set(gv) == set(G)
    for k in G:
      close(gv[k], G[k])
    _adam_ref(P, G, M, V, t, lr)
  got = {k: v.cpu().numpy() for k, v in eng.param_views().items()}
  assert set(got) == set(P) and got[('lat', 'w')].shape == (eng.hdim, D) and got[('lat', 'b')].shape == (D,)
  # every element of every parameter against the float64 trajectory
  for k in P:
    err, scale = float(np.abs(got[k] - P[k]).max()), max(1e-3, float(np.abs(P[k]).max()))
    print(f'{name} {k}: max error {err:.3e} = {err / scale:.3e} of the largest weight')
    assert err <= 2e-4 * scale, (k, err, scale)


@pytest.mark.gpu
@pytest.mark.parametrize('D', [5, 70])
def test_graph_replay_over_a_beta_schedule_equals_eager(D):
  """four steps under beta = 0.5, 1, 2, 4 with the noise drawn in the kernel: the captured step replays bit for bit what
  the eager launches compute -- klw and the step are read from device memory (the simulator has no graphs: GPU only, like
  the other models' replay tests)"""
  from tests.test_latent_regularizers import _Hip
  bk = _Hip()
  res = []
  for use_graph in (False, True):
    eng, P, x, n = relaxedbern_case(bk, tiny_spec(D), 6)
    xt = bk.T(x)
    outs = [eng.train_step(xt, None, lr=1e-3, beta=b, use_graph=use_graph).clone() for b in (0.5, 1.0, 2.0, 4.0)]
    sync(bk)
    res.append([eng.params.clone(), torch.stack(outs), eng.dp.clone(), eng.z.clone(), eng.eps.clone()])
  for a, b in zip(res[0], res[1]):
    assert torch.equal(a, b)
  klb = res[0][1][:, 2]   # (mean beta * kl: another noise and another beta at every step)
  assert bool(torch.isfinite(res[0][1]).all()) and len(set(klb.tolist())) == 4
  # a beta change between two replays of the SAME noise is seen: the KL term scales, the likelihood's does not, and
  # the projection's gradient is the one the eager backward forms under that klw
  eng, P, x, n = relaxedbern_case(bk, tiny_spec(D), 6)
  xt, nt = bk.T(x), bk.T(n)
  o1 = eng.train_step(xt, nt, lr=0.0, beta=1.0, use_graph=True).clone()
  dp1 = eng.dp.clone()
  o2 = eng.train_step(xt, nt, lr=0.0, beta=3.0, use_graph=True).clone()
  dp2 = eng.dp.clone()
  assert float(o1[1]) == float(o2[1]) and abs(float(o2[2]) - 3.0 * float(o1[2])) <= 1e-5 * abs(float(o2[2]))
  assert not torch.equal(dp1, dp2)
  eager, _, _, _ = relaxedbern_case(bk, tiny_spec(D), 6)
  eager.train_step(xt, nt, lr=0.0, beta=3.0)
  assert torch.equal(eager.dp, dp2)


# ---- 5. engine behaviour ------------------------------------------------------------------------------------------------
def test_refused_combinations(bk):
  enc, dec, in_shape, _ = tiny_spec()
  mk = lambda **kw: VAEEngine(enc, dec, in_shape, kw.pop('zdim', 5), 4, bk.dev, lib=bk.L,
                              latent_dist=kw.pop('latent_dist', 'relaxedbernoulli'), **kw)
  other = VAEEngine(enc, dec, in_shape, 5, 4, bk.dev, lib=bk.L)
  for kw, exc, word in ((dict(tc='betatc'), ValueError, 'tc'), (dict(latent_reg='mmd'), ValueError, 'mmd'),
                        (dict(latent_reg='dip_i'), ValueError, 'dip_i'), (dict(latent_reg='dip_ii'), ValueError, 'dip_ii'),
                        (dict(vamprior_components=3), ValueError, 'vamprior'),
                        (dict(vq_codes=5), ValueError, 'vq_codes'),
                        (dict(latent_cov='tril'), ValueError, 'tril'),
                        (dict(zdim=0), ValueError, 'zdim'), (dict(zdim=256), ValueError, 'zdim'),
                        (dict(temperature=0.0), ValueError, 'temperature'),
                        (dict(temperature=-0.5), ValueError, 'temperature'),
                        (dict(neck_bwd=True), NotImplementedError, 'neck_bwd'),
                        (dict(world_size=2), NotImplementedError, 'data parallel'),
                        (dict(force_dp=True), NotImplementedError, 'data parallel'),
                        (dict(range_words=other.range_words), NotImplementedError, 'range_words'),
                        (dict(analytic=True, reverse=False), NotImplementedError, 'reverse'),
                        (dict(latent_dist='bernoulli'), ValueError, 'latent_dist')):
    with pytest.raises(exc, match=word) as e:
      mk(**kw)
    if 'latent_dist' not in kw:
      assert 'relaxedbernoulli' in str(e.value), kw
  eng = mk(temperature=0.7)
  assert eng.temperature == 0.7 and eng.latent_dist == 'relaxedbernoulli'
  with pytest.raises(NotImplementedError, match='reverse'):
    eng.set_kl_form(True, reverse=False)
  assert mk(zdim=1).pw == 1 and mk(zdim=255).pw == 255


def test_step_is_the_unfused_slot_with_no_rng_launch(bk):
  spec = neck_spec(5, 128)
  assert VAEEngine(*spec, 2, bk.dev, lib=bk.L, neck=True).neck
  calls = []
  eng = VAEEngine(*spec, 2, bk.dev, lib=Recorder(bk.L, calls), neck=True, latent_dist='relaxedbernoulli')
  assert not (eng.neck or eng.lat_block) and eng.pw == 5
  x, _ = case_data(bk.dev, spec, B=2)
  calls.clear()
  eng.train_step(x, None, lr=1e-3, beta=2.0)   # (forward(fused=True): the default; the noise is drawn in the kernel)
  assert not [c for c in calls if 'neck' in c or 'latent_block' in c or 'odin_rng_' in c or 'concrete' in c
              or c in ('odin_latent_fwd', 'odin_latent_bwd')]
  assert calls.count('odin_latent_relaxedbern_fwd') == 1 and calls.count('odin_latent_relaxedbern_bwd') == 1
  i = calls.index('odin_latent_relaxedbern_fwd')
  assert calls[i - 1] == 'odin_dense_fwd'
  j = calls.index('odin_latent_relaxedbern_bwd')
  assert i < j and calls[j + 1:j + 3] == ['odin_dense_wgrad', 'odin_dense_bwd']
  # everything around the slot is what the sibling posterior's step launches (tiny_spec; the noise handed in)
  _, mine = launch_record(bk, latent_dist='relaxedbernoulli')
  _, sibling = launch_record(bk, latent_dist='relaxedonehot')
  assert [c.replace('relaxedbern', 'concrete') for c in mine] == sibling and 'odin_latent_relaxedbern_fwd' in mine
  assert bool(torch.isfinite(eng.out4).all()) and bool(torch.isfinite(eng.eps).all())
  assert bool(((eng.z > 0) & (eng.z < 1)).all())
  # the noise the step left behind is the stream of (seed, step)
  assert eng.step_count == 1 and np.array_equal(eng.eps.cpu().numpy().ravel(), rng_logistic(bk, 10, eng.seed, 1))


def test_plain_engine_call_list_is_unchanged(bk):
  eng, c1 = launch_record(bk)
  assert c1 == PLAIN_STEP_CALLS and eng.latent_dist == 'normal' and eng.pw == 2 * eng.D
  _, c2 = launch_record(bk, latent_dist='normal', temperature=0.5)
  assert c2 == PLAIN_STEP_CALLS
  nl = len(eng.enc_recs) + len(eng.dec_recs)
  assert eng.range_words.numel() == 2 * nl * RANGE_WORDS


# ---- 6. the model API ---------------------------------------------------------------------------------------------------
def relaxedbern_nets(D=5, C=1, alias='relaxedbernoulli', **kwargs):
  from odin_ai_amd.networks import RVconf
  nets = tiny_nets(C=C, zdim=D)
  nets['latents'] = RVconf(D, alias, projection=True, name='latents', kwargs=dict(kwargs))
  return nets


def api_x(B=6, seed=2):
  return np.clip(np.random.default_rng(seed).random((B, 8, 8, 1)), 1e-6, 1 - 1e-6).astype(np.float32)


def test_api_quick_start_builds_fits_and_returns_the_posterior(bk):
  from odin_ai_amd.vae import BetaVAE, RelaxedBernoulliPosterior
  D, tau = 5, 0.7
  vae = BetaVAE(beta=2.0, device=bk.dev, lib=bk.L, **relaxedbern_nets(D, alias='relaxedsigmoid', temperature=tau))
  x = api_x(8)
  before, _ = vae.optimize(x, training=False)
  vae.fit(x, max_iter=3, batch_size=8, learning_rate=1e-3, compile_graph=False)
  assert vae.step == 3 and np.isfinite(float(vae.optimize(x, training=False)[0])) and np.isfinite(float(before))
  n = np.random.default_rng(1).logistic(size=(8, D)).astype(np.float32)
  px, qz = vae(x, eps=n)
  assert isinstance(qz, RelaxedBernoulliPosterior) and qz.event_shape == (D,) and qz.batch_shape == (8,)
  assert qz.temperature == tau and qz.logits.shape == (8, D)
  assert torch.equal(qz.probs, torch.sigmoid(qz.logits))
  with pytest.raises(NotImplementedError):
    qz.mean()
  s = qz.sample(3, seed=1)
  assert s.shape == (3, 8, D) and torch.equal(s, qz.sample(3, seed=1)) and bool(((s >= 0) & (s <= 1)).all())
  assert qz.sample().shape == (8, D)
  # the posterior's own numbers against the restatement (the logits as the engine left them)
  l64, n64 = ru.t64(qz.logits.cpu().numpy()), ru.t64(n)
  u64, z64 = ru.relax(l64, n64, tau)
  z = qz.tensor()
  close(z.cpu().numpy(), z64.numpy())
  close(qz.log_prob(z).cpu().numpy(), ru.log_q(l64, u64, tau).numpy())
  # (at another point of the cube the logit is taken: a point well inside it)
  mid = torch.full_like(z, 0.3)
  u_mid = torch.full((8, D), math.log(0.3 / 0.7), dtype=F64)
  close(qz.log_prob(mid).cpu().numpy(), ru.log_q(l64, u_mid, tau).numpy())
  close(qz.KL_divergence(analytic=True).cpu().numpy(), ru.kl_bernoulli(l64).numpy())
  close(qz.KL_divergence(analytic=False).cpu().numpy(), ru.kl_mc(l64, n64, tau).numpy())
  fb = qz.KL_divergence(analytic=True, free_bits=0.4, keepdims=True)
  assert fb.shape == (1, 8) and float(fb.min()) >= 0.4 * D - 1e-6
  with pytest.raises(NotImplementedError, match='reverse'):
    qz.KL_divergence(analytic=True, reverse=False)
  # elbo_components: the engine's KL (times beta) is the wrapper's KL at the engine's sample
  llk, kl = vae.elbo_components(x, eps=n)
  _, q2 = vae.last_outputs
  assert llk['llk_image'].shape == (8,) and kl['kl_latents'].shape == (8,)
  close(kl['kl_latents'].cpu().numpy(), 2.0 * q2.KL_divergence(analytic=False).cpu().numpy())
  assert np.isfinite(vae.elbo(llk, kl).cpu().numpy()).all()
  assert vae.trainable_variables[('lat', 'w')].shape == (24, D) and vae.variable_name(('lat', 'w')) == 'latents/kernel'
  # the prior's samples: independent 0 / 1 entries, seeded
  zp = vae.sample_prior(7, seed=3)
  assert zp.shape == (7, D) and bool(((zp == 0) | (zp == 1)).all()) and 0 < float(zp.sum()) < 7 * D
  assert torch.equal(zp, vae.sample_prior(7, seed=3)) and not torch.equal(zp, vae.sample_prior(7, seed=4))
  assert vae.decode(zp, only_decoding=True).shape == (7, 8, 8, 1)
  assert vae.decode(qz, only_decoding=True).shape == (8, 8, 8, 1)


def test_marginal_log_prob_matches_float64_logmeanexp(bk):
  from odin_ai_amd.vae import VariationalAutoencoder
  from oracle.torch_ref import TorchVAE, t_seq
  D, ns, N, tau = 5, 3, 6, 0.5
  vae = VariationalAutoencoder(device=bk.dev, lib=bk.L, **relaxedbern_nets(D))
  x = api_x(N)
  n = np.random.default_rng(4).logistic(size=(ns, N, D)).astype(np.float32)
  llk, lat = vae.marginal_log_prob(x, n_mcmc=ns, reduce=None, batch_size=4, eps=n)
  T = {k: torch.as_tensor(v.cpu().numpy(), dtype=F64) for k, v in vae.trainable_variables.items()}
  x64 = torch.as_tensor(x, dtype=F64)
  h_e = t_seq(vae.encoder.layers, TorchVAE._sub(T, 'enc'), x64)
  l64 = (h_e @ T[('lat', 'w')] + T[('lat', 'b')])[None].expand(ns, N, D)
  u64, z64 = ru.relax(l64, ru.t64(n), tau)
  h_d = t_seq(vae.decoder.layers, TorchVAE._sub(T, 'dec'), z64.reshape(ns * N, D)).reshape((ns, N, 8, 8, 1))
  lme = lambda t: (torch.logsumexp(t, 0) - math.log(ns)).numpy()
  close(llk['image'].cpu().numpy(), lme((x64[None] * h_d - ru.softplus(h_d)).reshape(ns, N, -1).sum(-1)))
  close(lat['latents'][0].cpu().numpy(), lme(ru.log_q(l64, u64, tau)))
  close(lat['latents'][1].cpu().numpy(), lme(ru.log_p(z64)))
  # without explicit noise: drawn on the device, finite
  llk2, lat2 = vae.marginal_log_prob(x, n_mcmc=ns, reduce=None, batch_size=4)
  assert all(bool(torch.isfinite(t).all()) for t in (llk2['image'],) + tuple(lat2['latents']))


@pytest.mark.parametrize('fmt', ['npz', 'tf'])
def test_api_save_load_round_trip(bk, tmp_path, fmt):
  from odin_ai_amd.vae import BetaVAE
  vae = BetaVAE(beta=2.0, device=bk.dev, lib=bk.L, **relaxedbern_nets(5))
  x = api_x()
  vae.optimize(x, learning_rate=1e-2)
  path = str(tmp_path / 'w')
  vae.save_weights(path, save_format=fmt)
  other = BetaVAE(beta=2.0, device=bk.dev, lib=bk.L, seed=3, **relaxedbern_nets(5))
  assert not torch.equal(other.trainable_variables[('lat', 'w')], vae.trainable_variables[('lat', 'w')])
  other.load_weights(path, raise_notfound=True)
  assert other.step == 1
  for k, v in vae.trainable_variables.items():
    assert torch.equal(v, other.trainable_variables[k]), k
  n = np.random.default_rng(1).logistic(size=(6, 5)).astype(np.float32)
  a, b = vae.elbo_components(x, eps=n), other.elbo_components(x, eps=n)
  assert torch.equal(a[0]['llk_image'], b[0]['llk_image']) and torch.equal(a[1]['kl_latents'], b[1]['kl_latents'])


def test_api_supported_and_refused_classes(bk):
  from odin_ai_amd.networks import get_networks
  from odin_ai_amd.vae import get_vae
  x = api_x()
  for name, kw in (('vae', {}), ('betavae', dict(beta=2.0)), ('annealingvae', {}), ('betacapacityvae', {})):
    vae = get_vae(name)(device=bk.dev, lib=bk.L, **kw, **relaxedbern_nets(5))
    vae.fit(x, max_iter=2, batch_size=6, learning_rate=1e-3, compile_graph=False)
    eng = vae._engine(6)
    assert vae.step == 2 and eng.latent_dist == 'relaxedbernoulli' and eng.temperature == 0.5, name
    llk, kl = vae.elbo_components(x)
    assert llk['llk_image'].shape == (6,) and kl['kl_latents'].shape == (6,), name
    assert bool(torch.isfinite(llk['llk_image']).all()) and bool(torch.isfinite(kl['kl_latents']).all()), name
  for name in ('betatcvae', 'infovae', 'dipvae', 'vampriorvae', 'vqvae', 'factorvae'):
    with pytest.raises(ValueError, match='relaxedbernoulli'):
      get_vae(name)(device=bk.dev, lib=bk.L, **relaxedbern_nets(5))
  vae = get_vae('vae')(device=bk.dev, lib=bk.L, analytic=True, free_bits=0.3, sample_shape=(2,), **relaxedbern_nets(5))
  llk, kl = vae.elbo_components(x)
  assert llk['llk_image'].shape == (2, 6) and kl['kl_latents'].shape == (1, 6)
  assert float(kl['kl_latents'].min()) >= 0.3 * 5 - 1e-6
  assert np.isfinite(float(vae.optimize(x, learning_rate=1e-3)[0]))
  # reverse=False: at construction, in set_elbo_configs and in the engine's set_kl_form
  with pytest.raises(NotImplementedError, match='reverse'):
    vae.set_elbo_configs(reverse=False)
  with pytest.raises(NotImplementedError, match='reverse'):
    get_vae('vae')(device=bk.dev, lib=bk.L, analytic=True, reverse=False, **relaxedbern_nets(5))
  with pytest.raises(NotImplementedError, match='reverse'):
    vae._engine(6).set_kl_form(True, reverse=False)
  with pytest.raises(ValueError, match='temperature'):
    get_vae('vae')(device=bk.dev, lib=bk.L, **relaxedbern_nets(5, temperature=0.0))
  # the three aliases of the reference's table, and the dataset networks
  for alias in ('relaxedbern', 'relaxedsigmoid', 'relaxedbernoulli'):
    v = get_vae('vae')(device=bk.dev, lib=bk.L, **relaxedbern_nets(3, alias=alias))
    assert v._latent_dist_options() == dict(latent_dist='relaxedbernoulli', temperature=0.5), alias
  assert v._engine(2).latent_dist == 'relaxedbernoulli' and v._engine(2).pw == 3
  assert get_networks('dsprites', qz='relaxedbern')['latents'].posterior == 'relaxedbern'
  with pytest.raises(ValueError, match='relaxedbernoulli'):   # (the list of what is supported names the new posterior)
    get_vae('vae')(device=bk.dev, lib=bk.L, **relaxedbern_nets(3, alias='gumbel'))
