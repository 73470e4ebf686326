"""VampriorVAE (vamprior.hip, VAEEngine(vamprior_components=K), odin_ai_amd.vae.VampriorVAE) on both backends of the
`bk` fixture: the mixture kernel against a float64 numpy restatement of odin/bay/vi/autoencoder/vamprior.py:25-107,
whole training steps against float64 autograd (oracle.torch_ref.TorchVAE's layers, fed clip(W_u) a second time) and
the model API.  Tolerances: the standing bars of tests/test_latent_regularizers.py."""
import numpy as np
import pytest
import torch

from odin_ai_amd.engine import VAEEngine
from oracle import vae_oracle as vo
from oracle.torch_ref import TorchVAE, t_seq
from tests.engine_util import launch_record, neck_spec, tiny_batch, tiny_spec
from tests.range_audit import RangeAudit
from tests.test_latent_regularizers import (_adam_ref, _Hip, _st, api_nets, assert_grad, assert_value, np_softplus,
                                            oracle_params)

LO, HI = 1e-6, 1.0 - 1e-6
LOG2PI = float(np.log(2.0 * np.pi))


# ---- float64 restatement ----------------------------------------------------------------------------------------------
def np_vamp(z, pu):
  """c[B] = log N(z; 0, I) - log p(z), d(sum c)/dz, d(sum c)/dpu, log p(z)[B], responsibilities [B, K]"""
  z, pu = np.asarray(z, np.float64), np.asarray(pu, np.float64)
  K, D = pu.shape[0], pu.shape[1] // 2
  loc, raw = pu[:, :D], pu[:, D:]
  sg = np_softplus(raw)
  t = (z[:, None, :] - loc[None]) / sg[None]                       # [B, K, D]
  l = (-0.5 * t ** 2 - np.log(sg)[None] - 0.5 * LOG2PI).sum(-1)    # [B, K]
  m = l.max(1, keepdims=True)
  lse = m[:, 0] + np.log(np.exp(l - m).sum(1))
  logp = lse - np.log(K)
  c = (-0.5 * z ** 2 - 0.5 * LOG2PI).sum(-1) - logp
  r = np.exp(l - lse[:, None])
  dz = -z + (r[:, :, None] * t / sg[None]).sum(1)
  dloc = -(r[:, :, None] * t / sg[None]).sum(0)
  dsg = -(r[:, :, None] * (t ** 2 - 1.0) / sg[None]).sum(0)
  draw = dsg / (1.0 + np.exp(-raw))
  return c, dz, np.concatenate([dloc, draw], 1), logp, r


def run_vamp(bk, z, pu, coef=None, cgrad=None, grad=True):
  B, D = z.shape
  K = pu.shape[0]
  ws = bk.zeros(bk.L.odin_vamprior_workspace(B, K, D))
  c = bk.zeros(B)
  dz = bk.zeros(B, D) if grad else None
  dpu = bk.zeros(K, 2 * D) if grad else None
  zt, pt = bk.T(z), bk.T(pu)
  cf = bk.T(np.array([coef], np.float32)) if coef is not None else None
  cg = bk.T(np.array([cgrad], np.float32)) if cgrad is not None else None
  bk.L.odin_vamprior_fwd_bwd(zt.data_ptr(), pt.data_ptr(), ws.data_ptr(), c.data_ptr(),
                             dz.data_ptr() if grad else None, dpu.data_ptr() if grad else None,
                             cf.data_ptr() if cf is not None else None, cg.data_ptr() if cg is not None else None,
                             B, K, D, _st(bk.dev))
  return ws, c, dz, dpu


# ---- the kernel ------------------------------------------------------------------------------------------------------
VAMP_SIZES = [(2, 1, 1), (6, 5, 4), (256, 500, 10), (512, 500, 45), (300, 37, 64), (1030, 1024, 3)]


@pytest.mark.parametrize('scaled', [True, False])
@pytest.mark.parametrize('B,K,D', VAMP_SIZES)
def test_vamprior_kernel_matches_float64(bk, B, K, D, scaled):
  if bk.name == 'sim' and B * K * D > 400_000:
    B, K = min(B, 67), min(K, 131)   # (the CPU simulator: the same code on a smaller problem)
  rng = np.random.default_rng(B + K + D)
  z = (rng.standard_normal((B, D)) * 1.2 + 0.1).astype(np.float32)
  pu = np.concatenate([rng.standard_normal((K, D)) * 0.9, rng.standard_normal((K, D)) * 0.7 - 0.3], 1).astype(np.float32)
  coef, cgrad = (2.5, -1.5) if scaled else (None, None)
  ws, c, dz, dpu = run_vamp(bk, z, pu, coef, cgrad)
  rc, rdz, rdpu, _, _ = np_vamp(z, pu)
  cn = c.cpu().numpy()
  for b in range(B):
    assert_value(float(cn[b]), rc[b])
  assert_value(float(ws[0]) / (coef or 1.0), rc.mean())
  assert_grad(dz.cpu().numpy() / (cgrad or 1.0), rdz)
  assert_grad(dpu.cpu().numpy() / (cgrad or 1.0), rdpu)


def test_vamprior_kernel_limits(bk):
  z, pu = np.zeros((2, 3), np.float32), np.zeros((4, 6), np.float32)
  from odin_ai_amd._lib import OdinError
  ws, c = bk.zeros(64), bk.zeros(2)
  zt, pt = bk.T(z), bk.T(pu)
  for B, K, D in ((4097, 4, 3), (2, 1025, 3), (2, 4, 65), (0, 4, 3)):
    with pytest.raises(OdinError):
      bk.L.odin_vamprior_fwd_bwd(zt.data_ptr(), pt.data_ptr(), ws.data_ptr(), c.data_ptr(), None, None, None, None,
                                 B, K, D, _st(bk.dev))


# ---- conditioning ------------------------------------------------------------------------------------------------------
def test_vamprior_conditioning_far_and_narrow(bk):
  """softplus(raw) down to 1e-3 and |loc - z| up to 30: log densities near -4e8, where a sum of exponentials without
  the row maximum is -inf and float32 log densities would leave the responsibilities to rounding"""
  rng = np.random.default_rng(11)
  B, K, D = 9, 7, 6
  z = (rng.standard_normal((B, D)) * 2.0).astype(np.float32)
  loc = z[rng.integers(0, B, K)] + rng.uniform(-30.0, 30.0, (K, D))
  sg = 10.0 ** rng.uniform(-3.0, 0.0, (K, D))
  sg[0] = 1e-3
  raw = np.log(np.expm1(sg))
  pu = np.concatenate([loc, raw], 1).astype(np.float32)
  rc, rdz, rdpu, logp, _ = np_vamp(z, pu)
  assert logp.min() < -1e6 and np.abs(loc[None] - z[:, None]).max() > 25.0
  ws, c, dz, dpu = run_vamp(bk, z, pu)
  assert bool(torch.isfinite(c).all()) and bool(torch.isfinite(dz).all()) and bool(torch.isfinite(dpu).all())
  cn = c.cpu().numpy()
  for b in range(B):
    assert_value(float(cn[b]), rc[b])
  assert_grad(dz.cpu().numpy(), rdz)
  assert_grad(dpu.cpu().numpy(), rdpu)


def test_vamprior_single_standard_normal_component(bk):
  """K = 1 with the component N(0, I): the prior is the standard normal, c = 0 and no gradient reaches z"""
  rng = np.random.default_rng(12)
  B, D = 5, 4
  z = rng.standard_normal((B, D)).astype(np.float32)
  pu = np.concatenate([np.zeros((1, D)), np.full((1, D), np.log(np.expm1(1.0)))], 1).astype(np.float32)
  sg = np_softplus(pu[:, D:].astype(np.float64))   # (float32 raw: sigma = 1 to ~1e-7)
  ws, c, dz, dpu = run_vamp(bk, z, pu)
  bound = 4.0 * np.abs(sg - 1.0).max() * (1.0 + (z.astype(np.float64) ** 2).sum(1).max()) + 1e-7
  assert float(c.abs().max()) <= bound and abs(float(ws[0])) <= bound
  assert float(dz.abs().max()) <= 4.0 * np.abs(sg - 1.0).max() * np.abs(z).max() + 1e-7


def test_vamprior_identical_components(bk):
  """all components equal: responsibilities 1 / K -- log p is the one component's density, every component receives
  the same gradient, 1 / K of the single component's"""
  rng = np.random.default_rng(13)
  B, K, D = 6, 8, 3
  z = rng.standard_normal((B, D)).astype(np.float32)
  one = np.concatenate([rng.standard_normal((1, D)), rng.standard_normal((1, D))], 1).astype(np.float32)
  ws1, c1, dz1, dpu1 = run_vamp(bk, z, one)
  wsK, cK, dzK, dpuK = run_vamp(bk, z, np.repeat(one, K, 0))
  np.testing.assert_allclose(cK.cpu().numpy(), c1.cpu().numpy(), rtol=0, atol=2e-6)
  assert_grad(dzK.cpu().numpy(), dz1.cpu().numpy())
  for k in range(K):
    assert torch.equal(dpuK[k], dpuK[0])
  assert_grad(dpuK[0].cpu().numpy() * K, dpu1[0].cpu().numpy())
  _, _, _, _, r = np_vamp(z, np.repeat(one, K, 0))
  np.testing.assert_allclose(r, 1.0 / K, rtol=1e-12)


# ---- forward only / reproducible --------------------------------------------------------------------------------------
def test_vamprior_forward_only_and_reproducible(bk):
  rng = np.random.default_rng(14)
  B, K, D = 70, 33, 10
  z = rng.standard_normal((B, D)).astype(np.float32)
  pu = rng.standard_normal((K, 2 * D)).astype(np.float32)
  ws, c, dz, dpu = run_vamp(bk, z, pu, 1.5, 0.25)
  ws2, c2, dz2, dpu2 = run_vamp(bk, z, pu, 1.5, 0.25)
  assert torch.equal(ws[:1], ws2[:1]) and torch.equal(c, c2) and torch.equal(dz, dz2) and torch.equal(dpu, dpu2)
  wsf, cf, _, _ = run_vamp(bk, z, pu, 1.5, 0.25, grad=False)
  assert torch.equal(ws[:1], wsf[:1]) and torch.equal(c, cf)


# ---- whole steps against float64 autograd ----------------------------------------------------------------------------
def t_vamp_c(z, pu):
  K, D = pu.shape[0], pu.shape[1] // 2
  loc, sg = pu[:, :D], torch.nn.functional.softplus(pu[:, D:])
  l = (-0.5 * ((z[:, None, :] - loc[None]) / sg[None]) ** 2 - torch.log(sg)[None] - 0.5 * LOG2PI).sum(-1)
  logp = torch.logsumexp(l, 1) - float(np.log(K))
  return (-0.5 * z ** 2 - 0.5 * LOG2PI).sum(-1) - logp


def make_pseudoinputs(rng, K, n):
  """inside (0.05, 0.95), a few entries pushed outside [1e-6, 1 - 1e-6] (their gradient must be exactly 0)"""
  u = rng.uniform(0.05, 0.95, (K, n))
  flat = u.reshape(-1)
  idx = rng.choice(flat.size, size=min(6, flat.size // 2), replace=False)
  flat[idx] = np.array([-0.05, 1.2, 0.0, 1.0, -3.0, 5e-7])[:idx.size]
  return u.astype(np.float32), idx


def autograd_ref(spec, P, x, eps, beta, data_term=True, prior_term=True):
  """float64 loss and every gradient of mean(-llk + beta (kl_std + c)); ('vamp', 'u') in P is W_u"""
  enc, dec, in_shape, zdim = spec
  tv = TorchVAE(enc, dec, in_shape, zdim, beta=beta)
  T = tv.tensors(P)
  xt, et = torch.tensor(np.asarray(x), dtype=torch.float64), torch.tensor(np.asarray(eps), dtype=torch.float64)
  K = T[('vamp', 'u')].shape[0]
  cs = {}

  def extra(o):
    u = torch.clamp(T[('vamp', 'u')], LO, HI).reshape((K,) + tuple(in_shape))
    pu = t_seq(tv.enc, tv._sub(T, 'enc'), u) @ T[('lat', 'w')] + T[('lat', 'b')]
    cs['c'] = t_vamp_c(o['z'], pu)
    cs['pu'] = pu
    return beta * cs['c'].mean()
  out = tv.forward(T, xt, et, extra if prior_term else None)
  loss = out['loss'] if data_term else out['loss'] + out['elbo'].mean()
  loss.backward()
  G = {k: (v.grad.detach().numpy() if v.grad is not None else np.zeros(tuple(v.shape))) for k, v in T.items()}
  f = {k: (v.detach().numpy() if torch.is_tensor(v) else v) for k, v in out.items()}
  if prior_term:
    f['c'], f['pu'] = cs['c'].detach().numpy(), cs['pu'].detach().numpy()
  return f, G


def vamp_case(bk, spec, B, K, seed=7, **engkw):
  enc, dec, in_shape, zdim = spec
  rng = np.random.default_rng(seed)
  x = np.clip(rng.random((B,) + tuple(in_shape)), 1e-6, 1 - 1e-6)
  eps = rng.standard_normal((B, zdim))
  P = vo.OracleVAE(enc, dec, in_shape, zdim).init_params(seed=5)
  u, idx = make_pseudoinputs(rng, K, int(np.prod(in_shape)))
  P = dict(P)
  P[('vamp', 'u')] = u.astype(np.float64)
  eng = VAEEngine(enc, dec, in_shape, zdim, B, bk.dev, lib=bk.L, vamprior_components=K, **engkw)
  eng.load_params(P)
  return eng, P, x, eps, idx


def step_vs_autograd(bk, spec, B, K, beta=2.0, fused=True, tol=1e-4, **engkw):
  eng, P, x, eps, idx = vamp_case(bk, spec, B, K, **engkw)
  eng.step_count = 1
  eng.set_hyper(beta=beta)
  eng.forward(bk.T(x), bk.T(eps), fused=fused)
  eng.backward()
  if bk.dev.type == 'cuda':
    torch.cuda.synchronize()
  f, G = autograd_ref(spec, P, x, eps, beta)
  out4 = eng.out4.cpu().numpy()
  term = beta * float(f['c'].mean())
  assert abs(out4[3] - term) <= tol * max(1.0, abs(term)), (out4[3], term)
  assert abs(out4[0] - f['loss']) <= tol * max(1.0, abs(f['loss'])), (out4[0], f['loss'])
  assert np.abs(eng.llk.cpu().numpy() - f['llk']).max() <= tol * max(1.0, np.abs(f['llk']).max())
  klc = (eng.kl + eng.vamp_c).cpu().numpy() * beta
  ref = f['kl'] + beta * f['c']
  assert np.abs(klc - ref).max() <= tol * max(1.0, np.abs(ref).max())
  assert np.abs(eng.vamp_pu.cpu().numpy() - f['pu']).max() <= tol * max(1.0, np.abs(f['pu']).max())
  gv = {k: v.cpu().numpy() for k, v in eng.grad_views().items()}
  assert set(gv) == set(G)
  for k in G:
    err = np.abs(gv[k] - G[k]).max() / max(1e-30, np.abs(G[k]).max())
    assert err <= tol, (k, err)
  gu = gv[('vamp', 'u')].reshape(-1)
  assert np.all(gu[idx] == 0.0) and np.abs(gu).max() > 0.0
  return eng


@pytest.mark.parametrize('fused', [True, False])
def test_step_tiny_nets(bk, fused):
  """fused: the latent block's backward carries dz; otherwise odin_latent_bwd"""
  eng = step_vs_autograd(bk, tiny_spec(), 6, 5, fused=fused)
  assert eng._used_block == (fused and eng.lat_block) and not eng._used_neck
  assert eng._bwd_block() == (fused and eng.lat_block)
  if fused:
    assert eng.lat_block


@pytest.mark.parametrize('B,K', [(2, 3), (3, 2)])
def test_step_neck(bk, B, K):
  """odin_neck_bwd carries dz"""
  eng = step_vs_autograd(bk, neck_spec(5, 128), B, K)
  assert eng.neck and eng._used_neck and eng._bwd_neck()


def test_weight_gradients_are_the_sum_of_both_passes(bk):
  """beta large: the prior term is not lost in the likelihood's.  The engine's encoder gradients equal data pass +
  pseudo pass, each of which is also compared on its own (the pseudo pass alone: the gradient that reaches the encoder
  through pu and W_u only, from the float64 model with z detached from the encoder)."""
  spec, B, K, beta = tiny_spec(), 6, 5, 50.0
  eng = step_vs_autograd(bk, spec, B, K, beta=beta)
  _, P, x, eps, _ = vamp_case(bk, spec, B, K)
  f_all, G_all = autograd_ref(spec, P, x, eps, beta)
  # data pass alone: an engine without the prior, handed the same dz through extra_dz
  enc, dec, in_shape, zdim = spec
  plain = VAEEngine(enc, dec, in_shape, zdim, B, bk.dev, lib=bk.L)
  plain.load_params({k: v for k, v in P.items() if k[0] != 'vamp'})
  plain.step_count = 1
  plain.set_hyper(beta=beta)
  plain.forward(bk.T(x), bk.T(eps))
  plain.backward(extra_dz=eng.vamp_dz)
  gd = {k: v.cpu().numpy().astype(np.float64) for k, v in plain.grad_views().items()}
  ge = {k: v.cpu().numpy().astype(np.float64) for k, v in eng.grad_views().items()}
  # pseudo pass alone in float64: d(beta mean c)/d theta with z held fixed
  tv = TorchVAE(enc, dec, in_shape, zdim, beta=beta)
  T = tv.tensors(P)
  zt = torch.tensor(f_all['z'], dtype=torch.float64)
  u = torch.clamp(T[('vamp', 'u')], LO, HI).reshape((K,) + tuple(in_shape))
  pu = t_seq(tv.enc, tv._sub(T, 'enc'), u) @ T[('lat', 'w')] + T[('lat', 'b')]
  (beta * t_vamp_c(zt, pu).mean()).backward()
  differs = 0
  for k in gd:
    gp = T[k].grad.numpy() if T[k].grad is not None else np.zeros_like(gd[k])
    scale = max(1e-30, np.abs(G_all[k]).max())
    assert np.abs(gd[k] + gp - G_all[k]).max() <= 1e-4 * scale, k     # data + pseudo = the whole (float64 identity)
    # engine = its data pass + the float64 pseudo pass.  2e-4: the left side is the DIFFERENCE of two fp32 engine
    # results, each of which is held to the standing 1e-4 on its own (ge by step_vs_autograd above)
    assert np.abs(ge[k] - gd[k] - gp).max() <= 2e-4 * scale, k
    if k[0] in ('enc', 'lat'):
      differs += int(np.abs(gp).max() > 1e-3 * scale)
  assert differs >= 4   # (the pseudo pass matters in this case: dropping it would fail the comparison above)


# ---- three training steps against a float64 Keras-Adam trajectory ---------------------------------------------------------
def test_three_train_steps_follow_float64_adam(bk):
  """Parameters after three steps at the standing bar of the other models' Adam tests: 2e-4 of the tensor's largest
  weight, nothing added.  The tiny nets only: on neck_spec the bar is no measure of this feature -- Adam's first update
  is lr * sign(g) whatever |g| is, and the PLAIN engine (no prior) already sits at 0.87 of the bar there after ONE step
  on ('enc', 4, 'w') (3.7e-5 against 4.3e-5, CPU simulator); with the prior three steps measure 4.85e-5, 1.13 of the
  bar, on the same tensor.  The neck's gradients with the prior are held to 1e-4 by test_step_neck."""
  spec = tiny_spec()
  B, K, beta, lr = 4, 3, 2.0, 1e-3
  eng, P, x, eps, idx = vamp_case(bk, spec, B, K, hyper_ring_rows=16)
  u0 = P[('vamp', 'u')].copy()
  M = {k: np.zeros_like(v) for k, v in P.items()}
  V = {k: np.zeros_like(v) for k, v in P.items()}
  xt, et = bk.T(x), bk.T(eps)
  for t in (1, 2, 3):
    f, G = autograd_ref(spec, P, x, eps, beta)
    out = eng.train_step(xt, et, lr=lr, beta=beta).cpu().numpy()
    assert abs(out[0] - f['loss']) <= 1e-4 * max(1.0, abs(f['loss'])), (t, out[0], f['loss'])
    _adam_ref(P, G, M, V, t, lr)
  got = {k: v.cpu().numpy() for k, v in eng.param_views().items()}
  for k in P:
    assert np.abs(got[k] - P[k]).max() <= 2e-4 * max(1e-3, np.abs(P[k]).max()), k
  moved = np.abs(got[('vamp', 'u')] - u0)
  assert moved.max() > 1e-3 and np.all(moved.reshape(-1)[idx] == 0.0)   # W_u moves; the clipped entries do not


# ---- the plain step is the parent's ---------------------------------------------------------------------------------------
# Every library call of ONE train_step of a freshly built tiny_spec() engine (batch 4, no optional keyword), in order,
# recorded on the commit before VampriorVAE existed (the first step: the dry run of the fused reduction comes first).
PLAIN_STEP_CALLS = [
    'odin_conv2d_fwd', 'odin_conv2d_fwd', 'odin_dense_fwd_ranged', 'odin_latent_block_fwd', 'odin_deconv2d_fwd',
    'odin_deconv2d_fwd', 'odin_gaussian_head_fwd_bwd', 'odin_deconv2d_bwd', 'odin_deconv2d_bwd',
    'odin_latent_block_bwd', 'odin_dense_bwd_ranged', 'odin_conv2d_bwd', 'odin_conv2d_wgrad',
    'odin_wgrad_planes_defer_end', 'odin_slab_reduce_sumsq', 'odin_slab_reduce_sumsq', 'odin_adam_ring_parts']


def test_plain_step_issues_the_launches_it_issued_before(bk):
  """an engine built without any of the new keywords: the recorded call list of the commit before, first step and
  steady state (this test passes on that commit too)"""
  eng, c1 = launch_record(bk)
  assert c1 == PLAIN_STEP_CALLS
  _, c2 = launch_record(bk, steps=2)
  steady = list(PLAIN_STEP_CALLS)
  steady.remove('odin_slab_reduce_sumsq')   # (the dry run happens once)
  assert c2 == steady
  assert [e[0][0] for e in eng.layout.entries].count('vamp') == 0 and not hasattr(eng, 'penc')
  nl = len(eng.enc_recs) + len(eng.dec_recs)
  assert eng.range_words.numel() == 2 * nl * 2048


def test_vamprior_keyword_none_is_the_plain_engine_and_k_adds_the_pseudo_pass(bk):
  eng0, c0 = launch_record(bk)
  eng1, c1 = launch_record(bk, vamprior_components=None, pseudoinputs_mean=0.3, pseudoinputs_std=2.0)
  assert c1 == PLAIN_STEP_CALLS and eng1.vamp_K is None and not hasattr(eng1, 'penc')
  assert eng0.params.numel() == eng1.params.numel() and eng0.range_words.numel() == eng1.range_words.numel()
  # with K: the pseudo pass's launches appear, the parameter buffer grows by K * prod(in_shape)
  eng2, c2 = launch_record(bk, vamprior_components=3)
  assert c2.count('odin_vamprior_fwd_bwd') == 1 and c2.count('odin_clip_range_fwd') == 1
  assert c2.count('odin_clip_range_bwd') == 1 and c2.count('odin_slab_reduce') + c2.count('odin_slab_reduce_sumsq') >= 1
  assert eng2.layout.entries[-1][0] == ('vamp', 'u') and eng2.n_params == eng0.n_params + 3 * 64


# ---- range audit ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('spec_name', ['tiny', 'neck'])
def test_range_audit_three_steps(bk, spec_name):
  spec = tiny_spec() if spec_name == 'tiny' else neck_spec(5, 128)
  eng, P, x, eps, _ = vamp_case(bk, spec, 4, 3)
  audit = RangeAudit(eng)
  xt, et = bk.T(x), bk.T(eps)
  for _ in range(3):
    eng.train_step(xt, et, lr=1e-3, beta=2.0)
    audit.check_cleared()
  assert len(audit.steps) == 3 and audit.n_checked() > 0 and not audit.failures
  audit.check_cover()   # W_u's gradient arrives through a reduction job like every other tensor's
  # the pseudo pass's own words bound their tensors too (checked on a forward + backward without the clearing launch)
  eng.step_count = 1
  eng.set_hyper(beta=2.0)
  seen = []

  def check(e):
    e.penc.check_range_words()
    seen.append(int((e.penc.range_words != 0).sum()))
  eng.debug_check_ranges = check
  eng.forward(xt, et)
  eng.backward()
  assert seen and seen[0] > 0
  assert int((eng.range_words != 0).sum()) == 0


def test_excluded_options_raise_at_construction(bk):
  enc, dec, in_shape, zdim = tiny_spec()
  mk = lambda **kw: VAEEngine(enc, dec, in_shape, zdim, 4, bk.dev, lib=bk.L, vamprior_components=3, **kw)
  for kw, exc, word in ((dict(tc='betatc'), ValueError, 'tc'), (dict(latent_reg='mmd'), ValueError, 'latent_reg'),
                        (dict(analytic=True), NotImplementedError, 'analytic'),
                        (dict(analytic=True, reverse=False), NotImplementedError, 'reverse'),
                        (dict(free_bits=0.5), NotImplementedError, 'free_bits'),
                        (dict(capacity=True), NotImplementedError, 'capacity'),
                        (dict(force_dp=True), NotImplementedError, 'data parallel'),
                        (dict(world_size=2), NotImplementedError, 'data parallel')):
    with pytest.raises(exc, match=word):
      mk(**kw)
  with pytest.raises(ValueError, match='vamprior_components'):
    VAEEngine(enc, dec, in_shape, zdim, 4, bk.dev, lib=bk.L, vamprior_components=1025)
  with pytest.raises(ValueError, match='pseudoinputs'):
    mk(pseudoinputs=np.zeros((2, 64), np.float32))
  eng = mk(pseudoinputs_mean=0.4, pseudoinputs_std=0.05)
  w = eng.param_views()[('vamp', 'u')]
  assert w.shape == (3, 64) and abs(float(w.mean()) - 0.4) < 0.03 and 0.02 < float(w.std()) < 0.08


# ---- model API -------------------------------------------------------------------------------------------------------------
def _vamp_model(L, DEV, K=5, beta=2.0, **kw):
  from odin_ai_amd.vae import VampriorVAE
  rng = np.random.default_rng(21)
  u, idx = make_pseudoinputs(rng, K, 64)
  vae = VampriorVAE(n_components=K, pseudoinputs=u, beta=beta, device=DEV, lib=L, **api_nets(), **kw)
  return vae, u, idx


def test_api_names_and_defaults(bk):
  from odin_ai_amd.interpolation import Interpolation
  from odin_ai_amd.vae import BetaVAE, Vamprior, VampriorVAE, get_vae
  assert get_vae('vampriorvae') is VampriorVAE and get_vae('vamprior_vae') is VampriorVAE
  vae = VampriorVAE(n_components=7, device=bk.dev, lib=bk.L, **api_nets())
  assert isinstance(vae, BetaVAE) and vae.n_components == 7
  assert vae.pseudoinputs_mean == -0.05 and vae.pseudoinputs_std == 0.01
  assert isinstance(vae._beta, Interpolation) and abs(vae.beta - 1e-6) < 1e-9   # linear(1e-6 -> 1, 2000 steps) at step 0
  vae._step = 2000
  assert abs(vae.beta - 1.0) < 1e-6
  import inspect
  d = inspect.signature(VampriorVAE.__init__).parameters
  assert d['n_components'].default == 500
  assert isinstance(vae.vamprior, Vamprior) and vae.latents.prior is vae.vamprior and vae.vamprior.n_components == 7
  w = vae.trainable_variables[('vamp', 'u')]
  assert w.shape == (7, 64) and abs(float(w.mean()) + 0.05) < 0.005 and float(w.std()) < 0.02
  # the default initialisation lies below the clip: every pseudo-input is 1e-6 (the reference's behaviour, kept)
  assert float((vae.vamprior.pseudoinputs - 1e-6).abs().max()) < 1e-9


def test_api_elbo_and_optimize(bk):
  L, DEV = bk.L, bk.dev
  vae, u, idx = _vamp_model(L, DEV)
  x, eps = tiny_batch(2)
  spec = (api_nets()['encoder'].layers, api_nets()['decoder'].layers, (8, 8, 1), 4)
  P = oracle_params(vae)
  assert np.array_equal(P[('vamp', 'u')], u.astype(np.float64))
  f, _ = autograd_ref(spec, P, x.astype(np.float64), eps.astype(np.float64), 2.0)
  llk, kl = vae.elbo_components(x, eps=eps)
  assert set(kl) == {'kl_latents'} and kl['kl_latents'].shape == (6,)
  ref_kl = f['kl'] + 2.0 * f['c']
  assert np.abs(kl['kl_latents'].cpu().numpy() - ref_kl).max() <= 1e-4 * max(1.0, np.abs(ref_kl).max())
  elbo = vae.elbo(llk, kl).cpu().numpy()
  np.testing.assert_allclose(elbo, f['llk'] - ref_kl, rtol=1e-4, atol=1e-4)
  M = {k: np.zeros_like(v) for k, v in P.items()}
  V = {k: np.zeros_like(v) for k, v in P.items()}
  for t in (1, 2):
    f, G = autograd_ref(spec, P, x.astype(np.float64), eps.astype(np.float64), 2.0)
    loss, metrics = vae.optimize(x, eps=eps, learning_rate=1e-3)
    assert set(metrics) == {'llk_image', 'kl_latents'}
    assert abs(float(loss) - f['loss']) <= 1e-4 * max(1.0, abs(f['loss']))
    ref = float((f['kl'] + 2.0 * f['c']).mean())
    assert abs(float(metrics['kl_latents']) - ref) <= 1e-4 * max(1.0, abs(ref))
    _adam_ref(P, G, M, V, t, 1e-3)
  got = oracle_params(vae)
  for k in P:
    assert np.abs(got[k] - P[k]).max() <= 2e-4 * max(1e-3, np.abs(P[k]).max()), k
  assert vae.step == 2


def test_api_vamprior_distribution(bk):
  L, DEV = bk.L, bk.dev
  vae, u, idx = _vamp_model(L, DEV, K=5)
  P = oracle_params(vae)
  spec_enc = api_nets()['encoder'].layers
  T = {k: torch.tensor(v, dtype=torch.float64) for k, v in P.items()}
  uc = torch.clamp(T[('vamp', 'u')], LO, HI).reshape(5, 8, 8, 1)
  pu = (t_seq(spec_enc, TorchVAE._sub(T, 'enc'), uc) @ T[('lat', 'w')] + T[('lat', 'b')]).numpy()
  vp = vae.vamprior
  np.testing.assert_allclose(vp.pseudoinputs.cpu().numpy().reshape(5, -1), np.clip(u, LO, HI), rtol=0, atol=1e-7)
  np.testing.assert_allclose(vp.mean().cpu().numpy(), pu[:, :4], rtol=1e-4, atol=1e-5)
  np.testing.assert_allclose(vp.stddev().cpu().numpy(), np_softplus(pu[:, 4:]), rtol=1e-4, atol=1e-5)
  assert vp.distribution.loc.shape == (5, 4)
  z = np.random.default_rng(5).standard_normal((9, 4)).astype(np.float32)
  _, _, _, logp, _ = np_vamp(z, pu)
  got = vp.log_prob(z).cpu().numpy()
  assert np.abs(got - logp).max() <= 1e-4 * max(1.0, np.abs(logp).max())
  # any number of rows goes through the one batch-1 engine in chunks: no engine per row count, no 4096-row limit
  before = set(vae._engines)
  zz = np.random.default_rng(6).standard_normal((4100, 4)).astype(np.float32)
  got = vp.log_prob(zz).cpu().numpy()
  ref = np_vamp(zz, pu)[3]
  assert np.abs(got - ref).max() <= 1e-4 * max(1.0, np.abs(ref).max()) and set(vae._engines) == before


def test_api_sampling(bk):
  L, DEV = bk.L, bk.dev
  vae, u, idx = _vamp_model(L, DEV, K=6)
  # components far apart and narrow: push the projection's bias of the scale down and spread the means through W_u's
  # effect -- simpler: overwrite the latent projection so that loc depends strongly on the pseudo-input
  tv = vae.trainable_variables
  tv[('lat', 'w')][:, :4].mul_(40.0)
  tv[('lat', 'b')][4:].fill_(-8.0)
  tv[('lat', 'w')][:, 4:].zero_()
  vp = vae.vamprior
  loc = vp.mean().cpu().numpy()
  dmin = min(np.abs(loc[i] - loc[j]).max() for i in range(6) for j in range(i))
  sd = float(vp.stddev().max())
  assert dmin > 20.0 * sd, (dmin, sd)
  a, b = vp.sample(4, seed=3), vp.sample(4, seed=3)
  assert a.shape == (4, 4) and torch.equal(a, b) and not torch.equal(a, vp.sample(4, seed=4))
  near = np.abs(a.cpu().numpy()[:, None, :] - loc[None]).max(-1).argmin(1)
  assert len(set(near.tolist())) == 4                                     # n distinct components
  full = vp.sample(6, seed=1).cpu().numpy()
  assert sorted(np.abs(full[:, None, :] - loc[None]).max(-1).argmin(1).tolist()) == list(range(6))
  with pytest.raises(ValueError):
    vp.sample(7, seed=1)
  zp = vae.sample_prior(3, seed=9)
  assert zp.shape == (3, 4) and torch.equal(zp, vp.sample(3, seed=9))
  px = vae.sample_observation(3, seed=9)
  assert tuple(px.mean().shape) == (3, 8, 8, 1)


def test_api_marginal_log_prob_uses_the_mixture(bk):
  L, DEV = bk.L, bk.dev
  vae, u, idx = _vamp_model(L, DEV, K=5)
  x, _ = tiny_batch(2, 3)
  n = 4
  eps = np.random.default_rng(8).standard_normal((n, 3, 4)).astype(np.float32)
  llk, lat = vae.marginal_log_prob(x, n_mcmc=n, reduce=None, eps=eps)
  lq, lp = lat['latents']
  q = vae.encode(x)
  loc, sc = q.mean().cpu().numpy().astype(np.float64), q.stddev().cpu().numpy().astype(np.float64)
  z = loc[None] + sc[None] * eps.astype(np.float64)
  pu = vae.vamprior.distribution
  pu = np.concatenate([pu.loc.cpu().numpy(), pu.raw_scale.cpu().numpy()], 1)
  ref = np.stack([np_vamp(z[k], pu)[3] for k in range(n)])                 # [n, B]
  m = ref.max(0)
  ref_lme = m + np.log(np.exp(ref - m).mean(0))
  assert np.abs(lp.cpu().numpy() - ref_lme).max() <= 1e-4 * max(1.0, np.abs(ref_lme).max())
  assert lq.shape == (3,) and llk['image'].shape == (3,)


@pytest.mark.parametrize('fmt', ['npz', 'tf'])
def test_api_save_load_round_trip(bk, tmp_path, fmt):
  from odin_ai_amd.vae import VAMPRIOR_VARIABLE, VampriorVAE
  L, DEV = bk.L, bk.dev
  vae, u, idx = _vamp_model(L, DEV, K=5)
  x, eps = tiny_batch(2)
  vae.optimize(x, eps=eps, learning_rate=1e-2)
  path = str(tmp_path / 'w')
  vae.save_weights(path, save_format=fmt)
  assert vae.variable_name(('vamp', 'u')) == VAMPRIOR_VARIABLE
  other = VampriorVAE(n_components=5, beta=2.0, device=DEV, lib=L, **api_nets())
  assert not torch.equal(other.trainable_variables[('vamp', 'u')], vae.trainable_variables[('vamp', 'u')])
  other.load_weights(path, raise_notfound=True)
  assert other.step == 1
  for k, v in vae.trainable_variables.items():
    assert torch.equal(v, other.trainable_variables[k]), k
  a, b = vae.elbo_components(x, eps=eps), other.elbo_components(x, eps=eps)
  assert torch.equal(a[1]['kl_latents'], b[1]['kl_latents'])


def test_api_fit_and_excluded_options(bk):
  from odin_ai_amd.vae import VampriorVAE
  L, DEV = bk.L, bk.dev
  vae, u, idx = _vamp_model(L, DEV, K=4)
  xs = (np.random.default_rng(1).random((16, 8, 8, 1)) < 0.3).astype(np.float32)
  vae.fit(xs, max_iter=3, batch_size=8, learning_rate=1e-3, compile_graph=False)
  assert vae.step == 3
  _, m = vae.optimize(xs[:8], training=False)
  assert np.isfinite(float(m['kl_latents']))
  for kw in (dict(analytic=True), dict(free_bits=0.5), dict(sample_shape=2), dict(analytic=True, reverse=False)):
    with pytest.raises(NotImplementedError):
      VampriorVAE(n_components=4, device=DEV, lib=L, **api_nets(), **kw)
  with pytest.raises(NotImplementedError):
    vae.set_elbo_configs(analytic=True)


# ---- full size on the MI355X ----------------------------------------------------------------------------------------
GPU_CASES = [
    # name, spec, B, which latent forms run: (neck forward, neck backward)
    ('dsprites', lambda: vo.dsprites_spec(1), 256, (True, True)),
    ('shapes3d', lambda: vo.dsprites_spec(3), 256, (True, False)),
    ('celeba', lambda: vo.celeba_spec(45, 3), 512, (False, False)),
]


@pytest.mark.gpu
@pytest.mark.parametrize('name,spec,B,forms', GPU_CASES, ids=[c[0] for c in GPU_CASES])
def test_gpu_full_size_step(name, spec, B, forms):
  eng = step_vs_autograd(_Hip(), spec(), B, 500, beta=2.0)
  neck_f, neck_b = forms
  assert eng._used_neck == neck_f and eng._bwd_neck() == neck_b


@pytest.mark.gpu
def test_gpu_graph_replay_equals_eager():
  """three steps with the beta schedule in the device hyper ring: the captured step replays bit for bit what the
  eager launches compute"""
  bk = _Hip()
  spec = vo.dsprites_spec(1)
  enc, dec, in_shape, zdim = spec
  B, K = 256, 500
  rng = np.random.default_rng(1)
  xs = [bk.T(np.clip(rng.random((B,) + in_shape), 1e-6, 1 - 1e-6)) for _ in range(3)]
  sched = lambda t: dict(beta=1e-6 + (1.0 - 1e-6) * min(1.0, t / 4.0))
  res = []
  for use_graph in (False, True):
    eng, P, _, _, _ = vamp_case(bk, spec, B, K)
    outs, cs = [], []
    for x in xs:
      outs.append(eng.train_step(x, None, lr=1e-3, beta=1.0, use_graph=use_graph, schedule=sched).clone())
      cs.append(eng.vamp_c.clone())
    torch.cuda.synchronize()
    res.append((eng.params.clone(), torch.stack(outs), torch.stack(cs)))
  for a, b in zip(res[0], res[1]):
    assert torch.equal(a, b)
  assert bool(torch.isfinite(res[0][1]).all()) and float(res[0][1][:, 3].abs().min()) > 0
  u0 = bk.T(P[('vamp', 'u')]).reshape(-1)
  assert not torch.equal(res[0][0][eng.vamp_u_off:eng.vamp_u_off + u0.numel()], u0)   # W_u moved
