"""InfoVAE's maximum-mean discrepancy and DIPVAE's disentangled-inferred-prior penalty (latent_reg.hip) on both
backends of the `bk` fixture: the kernels against a float64 numpy restatement of odin/bay/vi/losses.py:39-98,
163-276, whole training steps against float64 autograd (oracle.torch_ref.TorchVAE with `extra_loss_fn`), and the
InfoVAE / DIPVAE model API."""
import functools

import numpy as np
import pytest
import torch

from odin_ai_amd.engine import PRIOR_KEY_SALT, VAEEngine
from odin_ai_amd.losses import disentangled_inferred_prior_loss, maximum_mean_discrepancy
from odin_ai_amd.vae import DIPVAE, BetaVAE, InfoVAE, MVNDiagPosterior, get_vae
from oracle import vae_oracle as vo
from oracle.torch_ref import TorchVAE
from tests.engine_util import neck_spec, tiny_batch, tiny_nets as api_nets, tiny_spec
from tests.parity_util import oracle_params


@pytest.fixture(scope='module')
def L(bk):
  return bk.L


@pytest.fixture(scope='module')
def DEV(bk):
  return bk.dev


def _st(dev):
  return torch.cuda.current_stream(dev).cuda_stream if torch.device(dev).type == 'cuda' else None


# ---- float64 restatements (losses.py) -----------------------------------------------------------------------------
def np_mmd(x, y, kernel):
  x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
  D = x.shape[1]

  def k(a, b):
    d = a[:, None, :] - b[None, :, :]
    if kernel == 'gaussian':
      return np.exp(-(d ** 2).sum(-1) / D)
    return np.abs(d.sum(-1))
  return k(x, x).mean() + k(y, y).mean() - 2.0 * k(x, y).mean()


def np_mmd_grad(x, y, kernel):
  """d MMD / dx (TF's sign(0) = 0 for the linear kernel)"""
  x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
  N, D = x.shape
  M = y.shape[0]

  def dk(a, b):   # [Na, Nb, D]: d k(a_i, b_j) / d a_i
    d = a[:, None, :] - b[None, :, :]
    if kernel == 'gaussian':
      return -2.0 / D * d * np.exp(-(d ** 2).sum(-1) / D)[..., None]
    return np.broadcast_to(np.sign(d.sum(-1))[..., None], d.shape)
  return 2.0 / N ** 2 * dk(x, x).sum(1) - 2.0 / (N * M) * dk(x, y).sum(1)


def np_softplus(v):
  return np.logaddexp(0.0, v)


def np_dip(p, only_mean, lo=2.0, ld=1.0):
  p = np.asarray(p, np.float64)
  D = p.shape[1] // 2
  mu, sc = p[:, :D], np_softplus(p[:, D:])
  N = mu.shape[0]
  c = mu - mu.mean(0)
  cov = c.T @ c / N
  if not only_mean:
    cov = cov + np.diag((sc ** 2).mean(0))
  off = cov - np.diag(np.diag(cov))
  val = lo * (off ** 2).sum() + ld * ((np.diag(cov) - 1.0) ** 2).sum()
  G = 2.0 * lo * off + np.diag(2.0 * ld * (np.diag(cov) - 1.0))
  dloc = 2.0 / N * c @ G
  dscale = np.zeros_like(sc) if only_mean else np.diag(G)[None, :] * 2.0 * sc / N
  return val, dloc, dscale


def assert_value(got, ref):
  assert abs(got - ref) <= max(2e-6, 1e-4 * abs(ref)), (got, ref)


def assert_grad(got, ref):
  got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
  scale = max(float(np.abs(ref).max()), 1e-30)
  assert float(np.abs(got - ref).max()) <= 1e-4 * scale, (float(np.abs(got - ref).max()), scale)


# ---- 1. kernels ---------------------------------------------------------------------------------------------------
MMD_SIZES = [(2, 1, 1), (6, 4, 100), (256, 10, 100), (512, 45, 100), (300, 64, 7)]


def run_mmd(bk, x, y, kernel, coef=None, cgrad=None, seed=0, step=None, grad=True):
  N, D = x.shape
  M = y.shape[0] if y is not None else None
  ws = bk.zeros(bk.L.odin_mmd_workspace(N, N, M, D))
  dz = bk.zeros(N, D) if grad else None
  xt = bk.T(x)
  yt = bk.T(y) if y is not None else None
  cf = bk.T(np.array([coef], np.float32)) if coef is not None else None
  cg = bk.T(np.array([cgrad], np.float32)) if cgrad is not None else None
  bk.L.odin_mmd_fwd_bwd(xt.data_ptr(), yt.data_ptr() if yt is not None else None, ws.data_ptr(),
                        dz.data_ptr() if grad else None, cf.data_ptr() if cf is not None else None,
                        cg.data_ptr() if cg is not None else None, N, M, D, {'gaussian': 0, 'linear': 1}[kernel],
                        seed, step.data_ptr() if step is not None else None, _st(bk.dev))
  return ws, dz


@pytest.mark.parametrize('kernel', ['gaussian', 'linear'])
@pytest.mark.parametrize('N,D,M', MMD_SIZES)
def test_mmd_kernel_matches_float64(bk, kernel, N, D, M):
  if bk.name == 'sim' and N * (N + M) * D > 2_000_000:
    N, M = min(N, 128), min(M, 50)   # (the CPU simulator: the same code on a smaller batch)
  rng = np.random.default_rng(N + D + M)
  x = (rng.standard_normal((N, D)) * 0.8 + 0.3).astype(np.float32)
  y = rng.standard_normal((M, D)).astype(np.float32)
  ws, dz = run_mmd(bk, x, y, kernel, coef=2.5, cgrad=-1.5)
  assert_value(float(ws[0]) / 2.5, np_mmd(x, y, kernel))
  assert_grad(dz.cpu().numpy() / -1.5, np_mmd_grad(x, y, kernel))
  # bit-reproducible; the workspace is left zeroed for the next launch
  assert float(ws[2:].abs().sum()) == 0.0
  ws2, dz2 = run_mmd(bk, x, y, kernel, coef=2.5, cgrad=-1.5)
  assert torch.equal(ws[:1], ws2[:1]) and torch.equal(dz, dz2)


def test_mmd_diagonal_and_identical_sets(bk):
  x = np.random.default_rng(3).standard_normal((5, 3)).astype(np.float32)
  ws, dz = run_mmd(bk, x, x.copy(), 'gaussian')
  # k(a, a) is exactly 1: MMD(x, x) = 0 exactly (the gradient's two passes cancel to rounding)
  assert float(ws[0]) == 0.0 and float(dz.abs().max()) <= 1e-12


@pytest.mark.parametrize('kernel', ['gaussian', 'linear'])
def test_mmd_in_kernel_prior_is_the_rng_normal_stream(bk, kernel):
  N, D, M = 20, 6, 37
  x = np.random.default_rng(4).standard_normal((N, D)).astype(np.float32)
  step = bk.T(np.array([7], np.int32), torch.int32)
  seed = 12345 | (3 << 32)
  y = bk.zeros(M, D)
  bk.L.odin_rng_normal(y.data_ptr(), M * D, seed, step.data_ptr(), _st(bk.dev))
  ws_a = bk.zeros(bk.L.odin_mmd_workspace(N, N, M, D))
  dz_a = bk.zeros(N, D)
  xt = bk.T(x)
  k = {'gaussian': 0, 'linear': 1}[kernel]
  bk.L.odin_mmd_fwd_bwd(xt.data_ptr(), None, ws_a.data_ptr(), dz_a.data_ptr(), None, None, N, M, D, k, seed,
                        step.data_ptr(), _st(bk.dev))
  ws_b, dz_b = run_mmd(bk, x, y.cpu().numpy(), kernel, seed=seed, step=step)
  assert torch.equal(ws_a[:1], ws_b[:1]) and torch.equal(dz_a, dz_b)
  assert_value(float(ws_a[0]), np_mmd(x, y.cpu().numpy(), kernel))
  # another step draws another prior sample
  step2 = bk.T(np.array([8], np.int32), torch.int32)
  ws_c = bk.zeros(8)
  bk.L.odin_mmd_fwd_bwd(xt.data_ptr(), None, ws_c.data_ptr(), None, None, None, N, M, D, k, seed, step2.data_ptr(),
                        _st(bk.dev))
  assert float(ws_c[0]) != float(ws_a[0])


def run_dip(bk, p, type2, ld=1.0, lo=2.0, cgrad=None):
  N, D2 = p.shape
  D = D2 // 2
  ws = bk.zeros(bk.L.odin_dip_workspace(1, D))
  dl, ds = bk.zeros(N, D), bk.zeros(N, D)
  cg = bk.T(np.array([cgrad], np.float32)) if cgrad is not None else None
  pt = bk.T(p)
  bk.L.odin_dip_fwd_bwd(pt.data_ptr(), ws.data_ptr(), dl.data_ptr(), ds.data_ptr(), None,
                        cg.data_ptr() if cg is not None else None, N, D, int(type2), ld, lo, _st(bk.dev))
  return ws, dl, ds


@pytest.mark.parametrize('far', [False, True])
@pytest.mark.parametrize('type2', [False, True])
@pytest.mark.parametrize('D', [1, 4, 10, 45])
def test_dip_kernel_matches_float64(bk, D, type2, far):
  N = 96 if bk.name == 'sim' else 512
  rng = np.random.default_rng(D * 7 + type2)
  p = np.concatenate([rng.standard_normal((N, D)) * 1.3 + 0.2 + (1e3 if far else 0.0),
                      rng.standard_normal((N, D)) * 0.5 - 0.5], 1).astype(np.float32)
  ws, dl, ds = run_dip(bk, p, type2, ld=1.5, lo=2.5, cgrad=0.75)
  val, rdl, rds = np_dip(p, not type2, lo=2.5, ld=1.5)
  assert_value(float(ws[0]), val)
  assert_grad(dl.cpu().numpy() / 0.75, rdl)
  if type2:
    assert_grad(ds.cpu().numpy() / 0.75, rds)
  else:
    assert float(ds.abs().max()) == 0.0
  ws2, dl2, ds2 = run_dip(bk, p, type2, ld=1.5, lo=2.5, cgrad=0.75)
  assert torch.equal(ws[:1], ws2[:1]) and torch.equal(dl, dl2) and torch.equal(ds, ds2)


def test_dip_moments_finish_equal_fused(bk):
  """the data-parallel pair (moments per rank | finish over the gathered blocks) on two halves of a batch"""
  N, D = 64, 5
  rng = np.random.default_rng(9)
  p = np.concatenate([rng.standard_normal((N, D)) + 3.0, rng.standard_normal((N, D))], 1).astype(np.float32)
  bs = 1 + 2 * D + D * D
  blocks = bk.zeros(2 * bs)
  pt = bk.T(p)
  for r in range(2):
    bk.L.odin_dip_moments(pt[r * N // 2:].data_ptr(), blocks[r * bs:].data_ptr(), N // 2, D, _st(bk.dev))
  val, rdl, rds = np_dip(p, False)
  for r in range(2):
    ws = bk.zeros(bk.L.odin_dip_workspace(2, D))
    dl, ds = bk.zeros(N // 2, D), bk.zeros(N // 2, D)
    bk.L.odin_dip_finish(blocks.data_ptr(), 2, pt[r * N // 2:].data_ptr(), ws.data_ptr(), dl.data_ptr(),
                         ds.data_ptr(), None, None, N // 2, D, 1, 1.0, 2.0, _st(bk.dev))
    assert_value(float(ws[0]), val)
    assert_grad(dl.cpu().numpy(), rdl[r * N // 2:(r + 1) * N // 2])
    assert_grad(ds.cpu().numpy(), rds[r * N // 2:(r + 1) * N // 2])


def test_standalone_losses(bk):
  rng = np.random.default_rng(5)
  B, D = 12, 3
  p = torch.tensor(rng.standard_normal((B, 2 * D)), dtype=torch.float32, device=bk.dev)
  z = torch.tensor(rng.standard_normal((B, D)), dtype=torch.float32, device=bk.dev)
  q = MVNDiagPosterior(p, z, D)
  y = rng.standard_normal((9, D)).astype(np.float32)
  for kernel in ('gaussian', 'linear'):
    v = maximum_mean_discrepancy(q, None, q_sample_shape=None, kernel=kernel, y=torch.tensor(y), lib=bk.L)
    assert_value(float(v), np_mmd(z.cpu().numpy(), y, kernel))
  v = maximum_mean_discrepancy(q, None, q_sample_shape=None, p_sample_shape=50, lib=bk.L)
  assert np.isfinite(float(v))
  for only_mean in (True, False):
    v = disentangled_inferred_prior_loss(q, only_mean=only_mean, lambda_offdiag=3.0, lambda_diag=0.5, lib=bk.L)
    assert_value(float(v), np_dip(p.cpu().numpy(), only_mean, lo=3.0, ld=0.5)[0])
  with pytest.raises(NotImplementedError):
    maximum_mean_discrepancy(q, None, q_sample_shape=None, kernel='polynomial', lib=bk.L)
  with pytest.raises(NotImplementedError):
    maximum_mean_discrepancy(q, None, q_sample_shape=4, lib=bk.L)


# ---- 2. whole training steps vs float64 autograd --------------------------------------------------------------------
def t_mmd(x, y, kernel='gaussian'):
  D = x.shape[1]

  def k(a, b):
    d = a[:, None, :] - b[None, :, :]
    return torch.exp(-(d ** 2).sum(-1) / D) if kernel == 'gaussian' else torch.abs(d.sum(-1))
  return k(x, x).mean() + k(y, y).mean() - 2.0 * k(x, y).mean()


def t_dip(loc, scale, only_mean, lo=2.0, ld=1.0):
  c = loc - loc.mean(0)
  cov = c.T @ c / loc.shape[0]
  if not only_mean:
    cov = cov + torch.diag((scale ** 2).mean(0))
  dg = torch.diagonal(cov)
  off = cov - torch.diag(dg)
  return lo * (off ** 2).sum() + ld * ((dg - 1.0) ** 2).sum()


REG = dict(mmd=dict(latent_reg='mmd', reg_coef=3.5, mmd_prior_samples=9),
           mmd_linear=dict(latent_reg='mmd', reg_coef=0.5, mmd_prior_samples=5, mmd_kernel='linear'),
           dip_i=dict(latent_reg='dip_i', reg_coef=1.0, dip_lambda=(1.5, 2.5)),
           dip_ii=dict(latent_reg='dip_ii', reg_coef=1.0, dip_lambda=(1.5, 2.5)))


def extra_loss(kw, y):
  reg, coef = kw['latent_reg'], kw['reg_coef']
  if reg == 'mmd':
    yt = torch.tensor(y, dtype=torch.float64)
    return lambda o: coef * t_mmd(o['z'], yt, kw.get('mmd_kernel', 'gaussian'))
  ld, lo = kw['dip_lambda']
  return lambda o: coef * t_dip(o['loc'], o['scale'], reg == 'dip_i', lo=lo, ld=ld)


def step_vs_autograd(bk, spec, B, kw, beta=2.0, analytic=False, fused=True, seed=7, tol=1e-4, **engkw):
  """one engine step (forward + backward) against float64 autograd of the same loss; returns the engine"""
  enc, dec, in_shape, zdim = spec
  rng = np.random.default_rng(seed)
  x = np.clip(rng.random((B,) + tuple(in_shape)), 1e-6, 1 - 1e-6)
  eps = rng.standard_normal((B, zdim))
  M = kw.get('mmd_prior_samples', 1)
  y = rng.standard_normal((M, zdim)).astype(np.float32)
  model = vo.OracleVAE(enc, dec, in_shape, zdim, beta=beta, analytic=analytic)
  P = model.init_params(seed=5)
  eng = VAEEngine(enc, dec, in_shape, zdim, B, bk.dev, lib=bk.L, analytic=analytic, **kw, **engkw)
  eng.load_params(P)
  eng.step_count = 1
  eng.set_hyper(beta=beta)
  prior = bk.T(y) if kw['latent_reg'] == 'mmd' else None
  eng.forward(bk.T(x), bk.T(eps), fused=fused, prior=prior)
  eng.backward()
  if bk.dev.type == 'cuda':
    torch.cuda.synchronize()
  tv = TorchVAE(enc, dec, in_shape, zdim, beta=beta, analytic=analytic)
  f, G = tv.loss_and_grads(P, x, eps, extra_loss_fn=extra_loss(kw, y))
  out4 = eng.out4.cpu().numpy()
  ref_term = float(f['loss'] + f['elbo'].mean())   # the extra term alone
  assert abs(out4[3] - ref_term) <= tol * max(1.0, abs(ref_term)), (out4[3], ref_term)
  assert abs(out4[0] - f['loss']) <= tol * max(1.0, abs(f['loss'])), (out4[0], f['loss'])
  assert np.abs(eng.llk.cpu().numpy() - f['llk']).max() <= tol * max(1.0, np.abs(f['llk']).max())
  assert np.abs(eng.kl.cpu().numpy() * beta - f['kl']).max() <= tol * max(1.0, np.abs(f['kl']).max())
  gv = {k: v.cpu().numpy() for k, v in eng.grad_views().items()}
  for k in G:
    err = np.abs(gv[k] - G[k]).max() / max(1e-30, np.abs(G[k]).max())
    assert err <= tol, (k, err)
  return eng


@pytest.mark.parametrize('reg', sorted(REG))
@pytest.mark.parametrize('fused,analytic', [(True, False), (False, True)])
def test_step_tiny_nets(bk, reg, fused, analytic):
  eng = step_vs_autograd(bk, tiny_spec(), 6, REG[reg], analytic=analytic, fused=fused)
  # fused: the latent block's forward and backward; otherwise the separate launches
  assert eng._used_block == (fused and eng.lat_block) and not eng._used_neck
  assert eng._bwd_block() == (fused and eng.lat_block)


@pytest.mark.parametrize('reg', ['mmd', 'dip_ii', 'dip_i'])
@pytest.mark.parametrize('B', [2, 3])
def test_step_neck(bk, reg, B):
  eng = step_vs_autograd(bk, neck_spec(5, 128), B, REG[reg])
  assert eng.neck and eng._used_neck and eng._bwd_neck()


def test_latent_reg_argument_errors(bk):
  enc, dec, in_shape, zdim = tiny_spec()
  with pytest.raises(ValueError):
    VAEEngine(enc, dec, in_shape, zdim, 4, bk.dev, lib=bk.L, tc='betatc', latent_reg='mmd')
  with pytest.raises(ValueError):
    VAEEngine(enc, dec, in_shape, zdim, 4, bk.dev, lib=bk.L, latent_reg='mivae')
  with pytest.raises(NotImplementedError):
    VAEEngine(enc, dec, in_shape, zdim, 4, bk.dev, lib=bk.L, latent_reg='mmd', mmd_kernel='polynomial')
  # the prior stream's key is not an eps key (seed < 2^32)
  eng = VAEEngine(enc, dec, in_shape, zdim, 4, bk.dev, lib=bk.L, latent_reg='mmd', prior_seed=1)
  assert eng.prior_key == 1 ^ PRIOR_KEY_SALT and eng.prior_key >> 32 != 0


# ---- 3. model API ---------------------------------------------------------------------------------------------------
def _adam_ref(P, G, M, V, t, lr):
  b1, b2, e = 0.9, 0.999, 1e-7
  a = lr * np.sqrt(1 - b2 ** t) / (1 - b1 ** t)
  for k in P:
    M[k] = b1 * M[k] + (1 - b1) * G[k]
    V[k] = b2 * V[k] + (1 - b2) * G[k] ** 2
    P[k] = P[k] - a * M[k] / (np.sqrt(V[k]) + e)


@pytest.mark.parametrize('which', ['info', 'info_linear', 'dip_ii', 'dip_i'])
def test_model_api(L, DEV, which):
  nets = api_nets()
  if which.startswith('info'):
    kernel = 'linear' if which == 'info_linear' else 'gaussian'
    div = functools.partial(maximum_mean_discrepancy, kernel=kernel, q_sample_shape=None, p_sample_shape=7)
    vae = InfoVAE(alpha=0.25, lamda=10.0, divergence=div, beta=123.0, device=DEV, lib=L, **nets)
    assert vae.beta == 0.75 and vae.alpha == 0.25
    coef, key, kw = 10.0 - 0.75, 'div_latents', dict(latent_reg='mmd', reg_coef=10.0 - 0.75, mmd_kernel=kernel)
  else:
    vae = DIPVAE(only_mean=which == 'dip_i', lambda_diag=1.5, lambda_offdiag=2.5, beta=2.0, device=DEV, lib=L, **nets)
    coef, key, kw = 1.0, 'dip_latents', dict(latent_reg=which, reg_coef=1.0, dip_lambda=(1.5, 2.5))
  beta = vae.beta
  x, eps = tiny_batch(2)
  eng = vae._engine(6)
  P = oracle_params(vae)
  tv = TorchVAE(nets['encoder'].layers, nets['decoder'].layers, (8, 8, 1), 4, beta=beta)
  prior = None
  if which.startswith('info'):
    # the step's prior sample: the stream the engine draws (prior_seed = the model's seed, step = vae.step)
    prior = torch.zeros(7, 4, device=DEV)
    step = torch.tensor([vae.step], dtype=torch.int32, device=DEV)
    L.odin_rng_normal(prior.data_ptr(), 28, eng.prior_key, step.data_ptr(), _st(DEV))
    prior = prior.cpu().numpy()
  kw['mmd_prior_samples'] = 7
  llk, kl = vae.elbo_components(x, eps=eps)
  assert set(kl) == {'kl_latents', key}
  f, _ = tv.loss_and_grads(P, x.astype(np.float64), eps.astype(np.float64), extra_loss_fn=extra_loss(kw, prior))
  term = float(f['loss'] + f['elbo'].mean())
  assert kl[key].dim() == 0
  assert abs(float(kl[key]) - term) <= 1e-4 * max(1.0, abs(term))
  elbo = vae.elbo(llk, kl).numpy(force=True)
  np.testing.assert_allclose(elbo, f['elbo'] - term, rtol=1e-4, atol=1e-4)
  # two optimize() steps against a float64 Keras-Adam trajectory (the prior sample of step t: stream step t - 1)
  M = {k: np.zeros_like(v) for k, v in P.items()}
  V = {k: np.zeros_like(v) for k, v in P.items()}
  for t in (1, 2):
    if which.startswith('info'):
      pr = torch.zeros(7, 4, device=DEV)
      step = torch.tensor([t], dtype=torch.int32, device=DEV)
      L.odin_rng_normal(pr.data_ptr(), 28, eng.prior_key, step.data_ptr(), _st(DEV))
      prior = pr.cpu().numpy()
    f, G = tv.loss_and_grads(P, x.astype(np.float64), eps.astype(np.float64), extra_loss_fn=extra_loss(kw, prior))
    loss, metrics = vae.optimize(x, eps=eps, learning_rate=1e-3)
    assert set(metrics) == {'llk_image', 'kl_latents', key}
    term = float(f['loss'] + f['elbo'].mean())
    assert abs(float(metrics[key]) - term) <= 1e-4 * max(1.0, abs(term)), (t, float(metrics[key]), term)
    assert abs(float(loss) - f['loss']) <= 1e-4 * max(1.0, abs(f['loss']))
    _adam_ref(P, G, M, V, t, 1e-3)
  got = oracle_params(vae)
  for k in P:
    assert np.abs(got[k] - P[k]).max() <= 2e-4 * max(1e-3, np.abs(P[k]).max()), k


def test_model_api_sample_shape_and_fit(L, DEV):
  vae = DIPVAE(beta=1.5, sample_shape=2, analytic=True, device=DEV, lib=L, **api_nets())
  x, eps = tiny_batch(2)
  eps2 = np.random.default_rng(3).standard_normal((12, 4)).astype(np.float32)
  llk, kl = vae.elbo_components(x, eps=eps2)
  assert llk['llk_image'].shape == (2, 6) and kl['dip_latents'].dim() == 0
  P = oracle_params(vae)
  tv = TorchVAE(api_nets()['encoder'].layers, api_nets()['decoder'].layers, (8, 8, 1), 4, beta=1.5, analytic=True)
  xx = np.concatenate([x, x]).astype(np.float64)
  f, _ = tv.loss_and_grads(P, xx, eps2.astype(np.float64),
                           extra_loss_fn=extra_loss(dict(latent_reg='dip_ii', reg_coef=1.0, dip_lambda=(1.0, 2.0)), None))
  term = float(f['loss'] + f['elbo'].mean())
  assert abs(float(kl['dip_latents']) - term) <= 1e-4 * max(1.0, abs(term))
  iv = InfoVAE(device=DEV, lib=L, **api_nets())
  xs = (np.random.default_rng(1).random((16, 8, 8, 1)) < 0.3).astype(np.float32)
  iv.fit(xs, max_iter=3, batch_size=8, learning_rate=1e-3, compile_graph=False)
  assert iv.step == 3
  _, m = iv.optimize(xs[:8], training=False)
  assert 'div_latents' in m and np.isfinite(float(m['div_latents']))


def test_model_api_errors_and_names(L, DEV):
  assert get_vae('infovae') is InfoVAE and get_vae('dipvae') is DIPVAE and get_vae('info_vae') is InfoVAE
  nets = api_nets()
  with pytest.raises(NotImplementedError):
    InfoVAE(divergence=functools.partial(maximum_mean_discrepancy, kernel='polynomial', q_sample_shape=None),
            device=DEV, lib=L, **nets)
  with pytest.raises(NotImplementedError):
    InfoVAE(divergence=functools.partial(maximum_mean_discrepancy, q_sample_shape=4), device=DEV, lib=L, **nets)
  with pytest.raises(NotImplementedError):
    InfoVAE(divergence=lambda q, p: 0.0, device=DEV, lib=L, **nets)
  vae = InfoVAE(device=DEV, lib=L, **nets)   # (no beta= keyword: the reference raises KeyError here, the port must not)
  assert vae.beta == 1.0 and vae.lamda == 100.0 and isinstance(vae, BetaVAE)


# ---- full size on the MI355X ----------------------------------------------------------------------------------------
class _Hip:
  name, dev = 'hip', torch.device('cuda:0')

  def __init__(self):
    from odin_ai_amd import _lib
    self.L = _lib.load()

  def T(self, a, dt=None):
    return torch.tensor(np.ascontiguousarray(a), dtype=dt or torch.float32, device=self.dev)


GPU_CASES = [
    # name, spec, B, which latent forms run: (neck forward, neck backward)
    ('dsprites', lambda: vo.dsprites_spec(1), 256, (True, True)),
    ('shapes3d', lambda: vo.dsprites_spec(3), 256, (True, False)),
    ('celeba', lambda: vo.celeba_spec(45, 3), 512, (False, False)),
]


@pytest.mark.gpu
@pytest.mark.parametrize('reg', ['mmd', 'dip_ii'])
@pytest.mark.parametrize('name,spec,B,forms', GPU_CASES, ids=[c[0] for c in GPU_CASES])
def test_gpu_full_size_step(name, spec, B, forms, reg):
  kw = dict(REG[reg])
  if reg == 'mmd':
    kw['mmd_prior_samples'] = 100
  eng = step_vs_autograd(_Hip(), spec(), B, kw, beta=1.0 if reg == 'mmd' else 2.0)
  neck_f, neck_b = forms
  assert eng._used_neck == neck_f and eng._bwd_neck() == neck_b


@pytest.mark.gpu
@pytest.mark.parametrize('reg', ['mmd', 'mmd_linear', 'dip_ii', 'dip_i'])
def test_gpu_graph_replay_equals_eager(reg):
  """three steps with the on-device prior sample and noise: the captured step replays bit for bit what the eager
  launches compute (hyper ring included)"""
  bk = _Hip()
  enc, dec, in_shape, zdim = vo.dsprites_spec(1)
  B = 256
  rng = np.random.default_rng(1)
  xs = [bk.T(np.clip(rng.random((B,) + in_shape), 1e-6, 1 - 1e-6)) for _ in range(3)]
  P = vo.OracleVAE(enc, dec, in_shape, zdim).init_params(seed=5)
  res = []
  for use_graph in (False, True):
    eng = VAEEngine(enc, dec, in_shape, zdim, B, bk.dev, lib=bk.L, **REG[reg])
    eng.load_params(P)
    outs = []
    for x in xs:
      outs.append(eng.train_step(x, None, lr=1e-3, beta=2.0, use_graph=use_graph).clone())
    torch.cuda.synchronize()
    res.append((eng.params.clone(), torch.stack(outs)))
  assert torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][1], res[1][1])
  assert bool(torch.isfinite(res[0][1]).all()) and float(res[0][1][:, 3].abs().min()) > 0
