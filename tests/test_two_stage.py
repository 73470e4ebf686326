"""TwoStageVAE (Dai & Wipf; two_stage_vae.py) on both backends of the `bk` fixture: the float64 restatement of
tests/twostage_util.py against torch.distributions, the two skip-head kernels of stage2.hip against that restatement,
whole stage-2 steps against float64 autograd, the untouched first stage, and the model API.

Tolerances are the project's own: 1e-4 of a tensor's maximum for values and gradients, 1e-9 for the restatement against
torch.distributions, 2e-4 of a tensor's largest weight for every parameter after three Adam steps; what the kernels
promise bit for bit (canaries, a second run, the range word) exactly.

Free bits "clamp some but not all samples": the threshold lies in the middle of the widest gap between two KL values of
the drawn batch (asserted: both kinds occur and no sample sits within twice the parity bound of it)."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

from odin_ai_amd._lib import OdinError
from odin_ai_amd.engine import RANGE_WORDS
from odin_ai_amd.vae import BetaVAE, MVNDiagPosterior, TwoStageVAE, get_vae
from tests import twostage_util as tu
from tests.engine_util import Recorder, tiny_nets

F64 = torch.float64
CANARY = -12345.5
ACTS = {'linear': 0, 'elu': 1, 'relu': 2}


def sync(bk):
  if bk.dev.type == 'cuda':
    torch.cuda.synchronize()


def ptr(t):
  return None if t is None else t.data_ptr()


# ---- 1. the restatement against torch.distributions ---------------------------------------------------------------------
@pytest.mark.parametrize('D', [1, 3, 10])
def test_restatement_matches_torch_distributions(D):
  from torch.distributions import Independent, Normal, kl_divergence
  g = torch.Generator().manual_seed(40 + D)
  loc, raw, eps, t = (torch.randn(6, D, generator=g, dtype=F64) for _ in range(4))
  scale = tu.softplus(raw)
  assert torch.allclose(scale, torch.nn.functional.softplus(raw), rtol=0, atol=1e-12)
  q = Independent(Normal(loc, scale), 1)
  p = Independent(Normal(torch.zeros(6, D, dtype=F64), torch.ones(6, D, dtype=F64)), 1)
  z = loc + scale * eps
  tol = dict(rtol=0, atol=1e-9)
  assert torch.allclose(tu.log_prob(loc, scale, t), q.log_prob(t), **tol)
  assert torch.allclose(tu.kl(loc, scale, z, 'mc'), q.log_prob(z) - p.log_prob(z), **tol)
  assert torch.allclose(tu.kl(loc, scale, z, 'analytic'), kl_divergence(q, p), **tol)
  assert torch.allclose(tu.kl(loc, scale, z, 'forward'), kl_divergence(p, q), **tol)


def test_restatement_concatenates_the_input_first():
  x, h = torch.tensor([[1.0, 2.0]], dtype=F64), torch.tensor([[10.0, 20.0, 30.0, 40.0]], dtype=F64)
  W = torch.arange(12, dtype=F64).reshape(6, 2)
  assert tu.skip_head(x, h, W, torch.zeros(2, dtype=F64)).tolist() == [[4 + 40 + 120 + 240 + 400, 1 + 6 + 50 + 140 + 270 + 440]]


# ---- 2. the heads against the restatement -------------------------------------------------------------------------------
def shifted(bk, a, shift):
  """the array on the device, `shift` floats behind a 16-byte boundary (the kernels' scalar-load instances)"""
  if not shift:
    return bk.T(a)
  buf = bk.zeros(a.size + 4)
  v = buf[shift:shift + a.size].view(a.shape)
  v.copy_(bk.T(a))
  assert v.data_ptr() % 16 == 4 * shift
  return v


def run_fwd(bk, x, h, W, b, mode, t=None, scale=1.0, pad=2, shift=0):
  """-> (p, llk, dp) as numpy, each with `pad` canary rows behind row B - 1"""
  B, Dx = x.shape
  H, N = h.shape[1], W.shape[1]
  xt, ht, Wt, bt = bk.T(x), shifted(bk, h, shift), shifted(bk, W, shift), bk.T(b)
  p, dp, llk = bk.full((B + pad, N), CANARY), bk.full((B + pad, N), CANARY), bk.full((B + pad,), CANARY)
  tt = bk.T(t) if t is not None else None
  sc = bk.T(np.array([scale], np.float32))
  bk.L.odin_skip_head_fwd(ptr(xt), ptr(ht), ptr(Wt), ptr(bt), ptr(p), mode, ptr(tt), ptr(sc) if mode else None,
                          ptr(llk) if mode else None, ptr(dp) if mode else None, B, Dx, H, N, None)
  sync(bk)
  return p.cpu().numpy(), llk.cpu().numpy(), dp.cpu().numpy()


def run_bwd(bk, x, h, W, dp, h_act, want_dx=True, pad=2, shift=0):
  """-> (dh, dx or None, slab rows [rows, K N + N], the range word's block as int32)"""
  B, Dx = x.shape
  H, N = h.shape[1], W.shape[1]
  K = Dx + H
  xt, ht, Wt, dpt = bk.T(x), shifted(bk, h, shift), shifted(bk, W, shift), bk.T(dp)
  rows = C.c_int(0)
  bk.L.odin_skip_head_bwd(None, None, None, None, ACTS[h_act], None, None, None, None, C.byref(rows), B, Dx, H, N, None)
  assert 1 <= rows.value <= 32 and rows.value <= bk.L.odin_max_slab_rows()
  slab = bk.full((rows.value + 1, K * N + N), CANARY)
  dh = bk.full((B + pad, H), CANARY)
  dx = bk.full((B + pad, Dx), CANARY) if want_dx else None
  word = bk.zeros(RANGE_WORDS, dtype=torch.int32)
  got = C.c_int(0)
  bk.L.odin_skip_head_bwd(ptr(xt), ptr(ht), ptr(Wt), ptr(dpt), ACTS[h_act], ptr(dh), ptr(word), ptr(dx), ptr(slab),
                          C.byref(got), B, Dx, H, N, None)
  sync(bk)
  assert got.value == rows.value
  return dh.cpu().numpy(), None if dx is None else dx.cpu().numpy(), slab.cpu().numpy(), word.cpu()


def ref_fwd(x, h, W, b, t, scale):
  """float64: p, llk [B], dp = -scale d(sum llk) / dp"""
  x, h, W, b, t = (torch.tensor(a, dtype=F64) for a in (x, h, W, b, t))
  p = tu.skip_head(x, h, W, b).detach().requires_grad_(True)
  E = p.shape[1] // 2
  llk = tu.log_prob(p[:, :E], tu.softplus(p[:, E:]), t)
  (-scale * llk.sum()).backward()
  return p.detach().numpy(), llk.detach().numpy(), p.grad.numpy()


def ref_bwd(x, h, W, dp, h_act):
  x, h, W, dp = (torch.tensor(a, dtype=F64) for a in (x, h, W, dp))
  Dx = x.shape[1]
  dh = (dp @ W[Dx:].T) * tu.act_grad_from_output(h_act, h)
  dx = dp @ W[:Dx].T
  return dh.numpy(), dx.numpy(), (torch.cat([x, h], -1).T @ dp).numpy(), dp.sum(0).numpy()


HEAD_B = [1, 5, 67]
HEAD_DE = [(1, 1), (6, 6), (10, 3), (45, 45), (128, 128)]
HEAD_H = [4, 36, 256, 1024]


@pytest.mark.parametrize('H', HEAD_H)
@pytest.mark.parametrize('Dx,E', HEAD_DE)
@pytest.mark.parametrize('B', HEAD_B)
def test_head_forward(bk, B, Dx, E, H):
  x, h, W, b, t, _ = tu.head_case(B, Dx, E, H, 'relu', 7 * B + Dx + H)
  scale = 1.0 / B
  p_ref, llk_ref, dp_ref = ref_fwd(x, h, W, b, t, scale)
  p0, llk0, dp0 = run_fwd(bk, x, h, W, b, 0)
  tu.close(p0[:B], p_ref)
  assert (p0[B:] == CANARY).all() and (llk0 == CANARY).all() and (dp0 == CANARY).all()   # mode 0 writes p only
  p1, llk1, dp1 = run_fwd(bk, x, h, W, b, 1, t, scale)
  assert np.array_equal(p1[:B], p0[:B])
  tu.close(llk1[:B], llk_ref)
  tu.close(dp1[:B], dp_ref)
  assert (p1[B:] == CANARY).all() and (llk1[B:] == CANARY).all() and (dp1[B:] == CANARY).all()
  again = run_fwd(bk, x, h, W, b, 1, t, scale)
  for a, c in zip((p1, llk1, dp1), again):
    assert np.array_equal(a, c)   # a fixed summation order: the same bits


@pytest.mark.parametrize('H', HEAD_H)
@pytest.mark.parametrize('Dx,E', HEAD_DE)
@pytest.mark.parametrize('B', HEAD_B)
def test_head_backward(bk, B, Dx, E, H):
  N, K = 2 * E, Dx + H
  for h_act in ('linear', 'elu', 'relu'):
    x, h, W, _, _, dp = tu.head_case(B, Dx, E, H, h_act, 11 * B + Dx + H)
    dh_ref, dx_ref, dW_ref, db_ref = ref_bwd(x, h, W, dp, h_act)
    dh, dx, slab, word = run_bwd(bk, x, h, W, dp, h_act)
    tu.close(dh[:B], dh_ref)
    tu.close(dx[:B], dx_ref)
    assert (dh[B:] == CANARY).all() and (dx[B:] == CANARY).all() and (slab[-1] == CANARY).all()
    tot = slab[:-1].astype(np.float64).sum(0)
    tu.close(tot[:K * N].reshape(K, N), dW_ref)
    tu.close(tot[K * N:], db_ref)
    # the range word: the bit pattern of max |dh|
    assert float(word.view(torch.float32).max()) == float(np.abs(dh[:B]).max())
    assert int(word.max()) == int(np.abs(dh[:B]).max().astype(np.float32).view(np.int32))
  # dx = NULL (the encoder side: x = z is data), and a second run gives the same bits
  dh2, none, slab2, word2 = run_bwd(bk, x, h, W, dp, h_act, want_dx=False)
  assert none is None and np.array_equal(dh2, dh) and np.array_equal(slab2, slab) and torch.equal(word2, word)


@pytest.mark.parametrize('Dx,E,H', [(1, 1, 4), (10, 3, 36), (45, 45, 1024), (7, 128, 256)])
def test_head_operands_off_a_16_byte_boundary(bk, Dx, E, H):
  """W and h one float behind a 16-byte boundary (views into a flat buffer): the instances with 4-byte loads"""
  B = 5
  x, h, W, b, t, dp = tu.head_case(B, Dx, E, H, 'elu', 17 + Dx)
  p_ref, llk_ref, dp_ref = ref_fwd(x, h, W, b, t, 0.5)
  p, llk, dpo = run_fwd(bk, x, h, W, b, 1, t, 0.5, shift=1)
  tu.close(p[:B], p_ref)
  tu.close(llk[:B], llk_ref)
  tu.close(dpo[:B], dp_ref)
  dh_ref, dx_ref, dW_ref, db_ref = ref_bwd(x, h, W, dp, 'elu')
  dh, dx, slab, _ = run_bwd(bk, x, h, W, dp, 'elu', shift=1)
  tu.close(dh[:B], dh_ref)
  tu.close(dx[:B], dx_ref)
  K, N = Dx + H, 2 * E
  tot = slab[:-1].astype(np.float64).sum(0)
  tu.close(tot[:K * N].reshape(K, N), dW_ref)
  tu.close(tot[K * N:], db_ref)
  assert (dh[B:] == CANARY).all() and (dx[B:] == CANARY).all() and (p[B:] == CANARY).all()


def test_head_backward_sums_a_chunk_in_rounds(bk):
  """more than 32 x 8 rows: a workgroup owns more than one round of 8 rows and adds the rounds into its slab row"""
  B, Dx, E, H = 261, 3, 2, 8
  x, h, W, _, _, dp = tu.head_case(B, Dx, E, H, 'elu', 5)
  dh_ref, dx_ref, dW_ref, db_ref = ref_bwd(x, h, W, dp, 'elu')
  dh, dx, slab, _ = run_bwd(bk, x, h, W, dp, 'elu')
  assert slab.shape[0] - 1 == 29
  tu.close(dh[:B], dh_ref)
  tu.close(dx[:B], dx_ref)
  tot = slab[:-1].astype(np.float64).sum(0)
  tu.close(tot[:(Dx + H) * 2 * E].reshape(Dx + H, 2 * E), dW_ref)
  tu.close(tot[(Dx + H) * 2 * E:], db_ref)
  assert (dh[B:] == CANARY).all() and (dx[B:] == CANARY).all()


@pytest.mark.parametrize('raw', [80.0, -80.0])
def test_head_scale_at_the_ends_of_its_range(bk, raw):
  """raw scales of +-80: softplus (80, e^-80) and its derivative stay finite.  At -80 the scale is 1.8e-35, so the
  target sits on the mean (any other residual squared leaves float32)."""
  B, Dx, E, H = 5, 6, 6, 36
  x, h, W, b, t, _ = tu.head_case(B, Dx, E, H, 'relu', 3)
  W[:, E:] = 0.0
  b[E:] = raw
  if raw < 0:
    W[:, :E] = 0.0
    t = np.tile(b[:E], (B, 1))
  p_ref, llk_ref, dp_ref = ref_fwd(x, h, W, b, t, 0.2)
  p, llk, dp = run_fwd(bk, x, h, W, b, 1, t, 0.2)
  assert np.isfinite(p[:B]).all() and np.isfinite(llk[:B]).all() and np.isfinite(dp[:B]).all()
  assert (p[:B, E:] == raw).all()
  tu.close(llk[:B], llk_ref)
  tu.close(dp[:B], dp_ref)
  if raw < 0:
    assert np.abs(dp[:B, E:]).min() > 0.19   # d llk / d raw = -sigmoid(raw) / softplus(raw) -> -1: not flushed to 0


def test_head_limits(bk):
  L = bk.L
  rows = C.c_int(0)

  def bwd(B, Dx, H, N, act=0):
    return L.odin_skip_head_bwd(None, None, None, None, act, None, None, None, None, C.byref(rows), B, Dx, H, N, None)

  buf = bk.zeros(4224 * 256)
  out = bk.zeros(256)

  def fwd(B, Dx, H, N, mode=0):
    return L.odin_skip_head_fwd(ptr(buf), ptr(buf), ptr(buf), ptr(buf), ptr(out), mode, None, None, None, None, B, Dx, H,
                                N, None)

  # every limit is served (the forward with real operands: one row)
  for Dx, H, N in ((1, 4, 2), (128, 4, 2), (1, 4096, 2), (1, 4, 256), (128, 4096, 256)):
    assert bwd(1, Dx, H, N) == 0 and rows.value == 1
    assert fwd(1, Dx, H, N) == 0
  sync(bk)
  # one past each of them: the bad-argument code
  for Dx, H, N in ((0, 4, 2), (129, 4, 2), (1, 0, 2), (1, 6, 2), (1, 4100, 2), (1, 4, 0), (1, 4, 3), (1, 4, 258)):
    for call in (bwd, fwd):
      with pytest.raises(OdinError, match=r'rc=-2'):
        call(1, Dx, H, N)
  for call in (bwd, fwd):
    with pytest.raises(OdinError, match=r'rc=-2'):
      call(0, 1, 4, 2)
  with pytest.raises(OdinError, match=r'rc=-2'):
    bwd(1, 1, 4, 2, act=3)
  with pytest.raises(OdinError, match=r'rc=-2'):
    fwd(1, 1, 4, 2, mode=2)
  with pytest.raises(OdinError, match=r'rc=-2'):
    fwd(1, 1, 4, 2, mode=1)   # mode 1 without target / scale / llk / dp


# ---- 3. whole stage-2 steps against float64 autograd --------------------------------------------------------------------
def make_model(bk, units=(8, 12), Du=None, cls=TwoStageVAE, lib=None, **kw):
  if cls is TwoStageVAE:
    kw = dict(stage2_units=units, stage2_zdim=Du, stage2_optimizer=dict(learning_rate=1e-3), **kw)
  return cls(device=bk.dev, lib=lib or bk.L, seed=3, **tiny_nets(zdim=5), **kw)


def batch(B, D=5, Du=5, seed=1):
  rng = np.random.default_rng(seed)
  x = np.clip(rng.random((B, 8, 8, 1)), 1e-6, 1 - 1e-6).astype(np.float32)
  return x, rng.standard_normal((B, D)).astype(np.float32), rng.standard_normal((B, Du)).astype(np.float32)


def first_stage_sample(vae, x, eps):
  """the cached sample of q(z|x), float64 (the frozen first stage is the kernels' own: stage 2 takes it as data)"""
  return vae.set_eval_stage(1).encode(x, eps=eps).z.detach().cpu().to(F64)


STEP_CASES = [  # units, Du, B, form, free bits
    ((8, 12), 5, 6, 'mc', False), ((8, 12), 3, 6, 'analytic', False), ((8, 12), 3, 6, 'forward', False),
    ((8, 12), 5, 6, 'mc', True), ((8, 12), 3, 6, 'analytic', True),
    # (two 256 x 256 layers on the two-plane GEMM, which wants 32 rows: the one case the simulator needs 13 s for)
    ((256, 256), 3, 32, 'mc', True)]


@pytest.mark.parametrize('units,Du,B,form,fb', STEP_CASES)
def test_stage2_steps(bk, units, Du, B, form, fb):
  vae = make_model(bk, units, Du, analytic=form != 'mc', reverse=form != 'forward')
  x, eps, eps2 = batch(B, 5, Du)
  z = first_stage_sample(vae, x, eps)
  net, n = vae.stage2, len(units)
  e2 = torch.tensor(eps2, dtype=F64)
  free_bits = None
  if fb:
    with torch.no_grad():
      _, _, k = tu.stage2_elbo(tu.params64(net, grad=False), z, e2, n, 'relu', form)
    free_bits = tu.gap_threshold(k.numpy(), 1e-4) / Du
    vae.set_elbo_configs(free_bits=free_bits)
  if units == (256, 256):   # (the 256 x 256 layers run on the two-plane GEMM: their backward reads the heads' range word)
    assert bk.L.odin_dense_reads_x_range(B, 256, 256)
  eng = vae._engine(B)
  frozen = [t.clone() for t in (eng.params, eng.m, eng.v)]
  vae.set_train_stage(2)
  P = {k: v.detach().numpy().copy() for k, v in tu.params64(net, grad=False).items()}
  M, V = {k: np.zeros_like(v) for k, v in P.items()}, {k: np.zeros_like(v) for k, v in P.items()}
  for t in range(1, 4):
    Pt = {k: torch.tensor(v, dtype=F64, requires_grad=True) for k, v in P.items()}
    loss, ll, k = tu.stage2_elbo(Pt, z, e2, n, 'relu', form, free_bits)
    loss.backward()
    if fb and t == 1:
      clamped = (k.detach().numpy() == free_bits * Du)
      assert clamped.any() and not clamped.all()
    got_loss, metrics = vae.optimize(x, training=True, eps=eps, eps2=eps2, track_gradients=True)
    sync(bk)
    if t == 1:   # (later steps start from parameters that agree to 2e-4 only)
      tu.close(float(got_loss), loss.item())
      tu.close(float(metrics['llk_latents']), ll.mean().item())
      tu.close(float(metrics['kl_latents2']), k.mean().item())
      for name in P:
        tu.close(metrics['_grad/' + name].cpu().numpy(), Pt[name].grad.numpy())
    tu.adam_ref(P, {k: v.grad.numpy() for k, v in Pt.items()}, M, V, t, 1e-3)
  assert net.t == 3 and vae.step == 3
  got = tu.flat_views(net, net.params)
  for name in P:
    assert np.abs(got[name] - P[name]).max() <= 2e-4 * np.abs(P[name]).max(), name
  # the first stage is frozen: parameters and Adam state keep their bits
  for a, b in zip((eng.params, eng.m, eng.v), frozen):
    assert torch.equal(a, b)


def test_stage2_nan_policy(bk):
  vae = make_model(bk).set_train_stage(2)
  x, eps, eps2 = batch(6)
  net = vae.stage2
  net.params[net.lat_b_off] = float('nan')   # (a bias of Latents2: a relu would swallow a NaN below it)
  keep = torch.ones_like(net.params, dtype=torch.bool)
  keep[net.lat_b_off] = False
  before = [t.clone() for t in (net.params, net.m, net.v)]
  vae.optimize(x, eps=eps, eps2=eps2, nan_gradients_policy='skip')
  sync(bk)
  assert vae.nan_flag and net.t == 1
  for a, b in zip((net.params, net.m, net.v), before):
    assert torch.equal(a[keep], b[keep])   # the update was skipped on the device
  net.flag.zero_()
  vae.optimize(x, eps=eps, eps2=eps2, nan_gradients_policy='ignore')
  sync(bk)
  assert not vae.nan_flag and not torch.equal(net.m[keep], before[1][keep])


# ---- 4. stage 1 is a BetaVAE ----------------------------------------------------------------------------------------------
def test_stage1_is_the_beta_vae(bk):
  x, eps, _ = batch(2)
  runs = []
  for cls in (BetaVAE, TwoStageVAE):
    calls = []
    vae = make_model(bk, cls=cls, lib=Recorder(bk.L, calls, args=True), beta=2.5)
    losses = [vae.optimize(x, training=True, eps=eps, learning_rate=1e-3)[0].clone() for _ in range(2)]
    sync(bk)
    runs.append((calls, losses, vae._engine(2).params.clone()))
  (c0, l0, p0), (c1, l1, p1) = runs
  assert c0 == c1 and len(c0) > 0
  assert all(torch.equal(a, b) for a, b in zip(l0, l1)) and torch.equal(p0, p1)


# ---- 5. the model API ---------------------------------------------------------------------------------------------------
def test_get_vae():
  assert get_vae('twostagevae') is TwoStageVAE and get_vae('two_stage_vae') is TwoStageVAE


def test_elbo_components_in_both_stages(bk):
  vae = make_model(bk, Du=3, beta=4.0)
  x, eps, eps2 = batch(6, 5, 3)
  llk, kl = vae.elbo_components(x, eps=eps)
  assert list(llk) == ['llk_image'] and list(kl) == ['kl_latents']
  assert tuple(llk['llk_image'].shape) == (6,) and tuple(kl['kl_latents'].shape) == (6,)
  vae.set_train_stage(2)
  llk, kl = vae.elbo_components(x, eps=eps, eps2=eps2)
  assert list(llk) == ['llk_latents'] and list(kl) == ['kl_latents2']
  assert tuple(llk['llk_latents'].shape) == (6,) and tuple(kl['kl_latents2'].shape) == (6,)
  # beta is not applied in stage 2, and the loss of the evaluation step is -mean(llk - kl)
  z = first_stage_sample(vae, x, eps)
  _, ll, k = tu.stage2_elbo(tu.params64(vae.stage2, grad=False), z, torch.tensor(eps2, dtype=F64), 2, 'relu')
  tu.close(llk['llk_latents'].cpu().numpy(), ll.numpy())
  tu.close(kl['kl_latents2'].cpu().numpy(), k.numpy())
  loss, _ = vae.optimize(x, training=False, eps=eps, eps2=eps2)
  tu.close(float(loss), float(-(ll - k).mean()))
  assert vae.stage2.t == 0 and vae.step == 0


def test_encode_two_stages(bk):
  vae = make_model(bk, Du=3)
  x, eps, eps2 = batch(6, 5, 3)
  eps3 = np.random.default_rng(9).standard_normal((6, 5)).astype(np.float32)
  qz_x, qu_z, qz_u = vae.encode_two_stages(x, eps=eps, eps2=eps2, eps3=eps3)
  assert all(isinstance(q, MVNDiagPosterior) for q in (qz_x, qu_z, qz_u))
  assert qz_x.event_shape == (5,) and qu_z.event_shape == (3,) and qz_u.event_shape == (5,)
  assert qz_x.batch_shape == qu_z.batch_shape == qz_u.batch_shape == (6,)
  assert tuple(qu_z.tensor().shape) == (6, 3) and tuple(qz_u.tensor().shape) == (6, 5)
  # eval stage 2: encode returns q(z|u), against the restatement
  assert isinstance(vae.set_eval_stage(1).encode(x, eps=eps), MVNDiagPosterior)
  he = vae.set_eval_stage(2).encode(x, only_encoding=True)
  assert torch.is_tensor(he) and tuple(he.shape) == (6, 24)   # passed through unchanged
  q = vae.encode(x, eps=eps, eps2=eps2, eps3=eps3)
  P = tu.params64(vae.stage2, grad=False)
  z = qz_x.z.detach().cpu().to(F64)
  loc2, sc2 = tu.posterior2(P, z, 2, 'relu')
  u = loc2 + sc2 * torch.tensor(eps2, dtype=F64)
  loc, sc = tu.likelihood2(P, u, 2, 'relu')
  tu.close(qu_z.tensor().cpu().numpy(), u.numpy())
  tu.close(q.mean().cpu().numpy(), loc.numpy())
  tu.close(q.stddev().cpu().numpy(), sc.numpy())
  tu.close(q.tensor().cpu().numpy(), (loc + sc * torch.tensor(eps3, dtype=F64)).numpy())
  assert torch.equal(q.tensor(), qz_u.tensor())
  vae.set_eval_stage(1)


def test_sample_prior(bk):
  vae = make_model(bk, Du=3)
  a, b, c = vae.sample_prior(7, seed=5), vae.sample_prior(7, seed=5, two_stage=True), vae.sample_prior(7, seed=6)
  assert tuple(a.shape) == (7, 5) and torch.equal(a, b) and not torch.equal(a, c)
  assert bool(torch.isfinite(a).all())
  plain = vae.sample_prior(7, seed=5, two_stage=False)
  g = torch.Generator(device='cpu').manual_seed(5)
  assert torch.equal(plain.cpu(), torch.randn(7, 5, generator=g))
  px = vae.sample_observation(3, seed=2)
  assert px.batch_shape == (3,) and px.event_shape == (8, 8, 1)


def test_fit_trains_both_stages(bk):
  x = np.clip(np.random.default_rng(4).random((6, 8, 8, 1)), 1e-6, 1 - 1e-6).astype(np.float32)
  vae = make_model(bk, stage2_iter_ratio=2)
  vae.fit(x, max_iter=3, batch_size=2, compile_graph=False)
  assert vae.stage2.t == 6 and vae.train_stage == 1 and vae.step == 9
  off = make_model(bk, stage2_iter_ratio=2, auto_train_2stages=False)
  off.fit(x, max_iter=1, batch_size=2, compile_graph=False)
  assert off.stage2.t == 0 and off.train_stage == 1 and off.step == 1


def test_checkpoint_round_trip(bk, tmp_path):
  x, eps, eps2 = batch(6)
  a = make_model(bk).set_train_stage(2)
  for _ in range(2):
    a.optimize(x, eps=eps, eps2=eps2)
  path = str(tmp_path / 'two_stage')
  a.save_weights(path)
  b = make_model(bk).set_train_stage(2)
  b.load_weights(path, raise_notfound=True)
  assert b.stage2.t == 2 and b.step == 2
  for name in ('params', 'm', 'v'):
    assert torch.equal(getattr(a.stage2, name), getattr(b.stage2, name)), name
  names = set(a._extra_checkpoint_variables())
  for want in ('encoder2/Encoder2_0/kernel', 'encoder2/Encoder2_1/bias', 'latents2/kernel', 'latents2/bias',
               'decoder2/Decoder2_0/kernel', 'decoder2/Decoder2_1/bias', 'observation2/kernel', 'observation2/bias',
               'stage2_optimizer/latents2/kernel/m', 'stage2_optimizer/decoder2/Decoder2_0/bias/v',
               'stage2_optimizer/iter'):
    assert want in names, want
  la, _ = a.optimize(x, eps=eps, eps2=eps2)
  lb, _ = b.optimize(x, eps=eps, eps2=eps2)
  sync(bk)
  assert torch.equal(la, lb) and a.stage2.t == b.stage2.t == 3
  for name in ('params', 'm', 'v'):
    assert torch.equal(getattr(a.stage2, name), getattr(b.stage2, name)), name


def test_refusals(bk):
  from odin_ai_amd.networks import RVconf
  for post in ('mvntril', 'relaxedonehot', 'relaxedbern'):
    nets = tiny_nets(zdim=5)
    nets['latents'] = RVconf((5,), post, projection=True, name='latents')
    with pytest.raises(ValueError, match='mvndiag'):
      TwoStageVAE(device=bk.dev, lib=bk.L, stage2_units=(8, 12), **nets)
  for units, word in (((8, 10), r'stage2_units\[-1\] = 10'), ((6, 8), r'stage2_units\[0\] = 6'),
                      ((8, 4100), r'4096'), ((), 'at least one')):
    with pytest.raises(ValueError, match=word):
      make_model(bk, units=units)
  with pytest.raises(ValueError, match='stage2_zdim = 129'):
    make_model(bk, Du=129)
  x, eps, _ = batch(6)
  vae = make_model(bk, sample_shape=(2,)).set_train_stage(2)
  with pytest.raises(NotImplementedError, match='sample_shape'):
    vae.optimize(x, eps=eps)
  with pytest.raises(NotImplementedError, match='sample_shape'):
    vae.elbo_components(x)
  dp = make_model(bk).set_train_stage(2)
  dp.force_dp = True
  with pytest.raises(NotImplementedError, match='data parallel'):
    dp.optimize(x, eps=eps)
  with pytest.raises(NotImplementedError, match='clipnorm'):
    make_model(bk).set_train_stage(2).optimize(x, eps=eps, global_clipnorm=1.0)
  with pytest.raises(ValueError, match='stage'):
    make_model(bk).set_train_stage(3)


# ---- 6. full size (the GPU only) ----------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_full_size_step_on_the_gpu():
  """the dSprites stack at B = 256, D = 10, units (1024,) * 3: one stage-2 step against float64 autograd"""
  from odin_ai_amd import _lib
  from odin_ai_amd.networks import get_networks
  assert torch.cuda.is_available()
  vae = TwoStageVAE(device='cuda:0', lib=_lib.load(), seed=2, stage2_optimizer=dict(learning_rate=1e-3),
                    **get_networks('dsprites'))
  assert vae.zdim == 10 and vae.stage2_units == (1024, 1024, 1024)
  rng = np.random.default_rng(0)
  x = (rng.random((256, 64, 64, 1)) < 0.2).astype(np.float32)
  eps, eps2 = (rng.standard_normal((256, 10)).astype(np.float32) for _ in range(2))
  z = first_stage_sample(vae, x, eps)
  Pt = tu.params64(vae.stage2)
  loss, ll, k = tu.stage2_elbo(Pt, z, torch.tensor(eps2, dtype=F64), 3, 'relu')
  loss.backward()
  vae.set_train_stage(2)
  got, metrics = vae.optimize(x, eps=eps, eps2=eps2, track_gradients=True)
  torch.cuda.synchronize()
  tu.close(float(got), loss.item())
  tu.close(float(metrics['llk_latents']), ll.mean().item())
  tu.close(float(metrics['kl_latents2']), k.mean().item())
  for name, p in Pt.items():
    tu.close(metrics['_grad/' + name].cpu().numpy(), p.grad.numpy())
  assert vae.stage2.t == 1 and not vae.nan_flag
