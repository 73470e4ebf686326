"""The count observations ('nb' / 'zinb'), LogNorm and the gene-expression stacks: the float64 restatement against
torch.distributions, the HIP kernels against the restatement, whole training steps against float64 autograd, the launch
lists, data parallelism and the model API.

Kernel bounds: an element's error is measured in units of 2^-24 times the sum of the magnitudes of its terms (M, Mg, Ml,
Mz of tests/nb_util.py) and capped at 32 of them.  The cap is a condition, not a measurement: a float32 evaluation of the
difference forms stays below 9, the literal lgamma(r + x) - lgamma(r) in float32 exceeds 1000 on the same inputs
(test_literal_float32_formula_misses_the_bound shows it on the CPU).  Measured on an MI355X and on the simulator alike
(the element function is float64): 0.95 units for 'nb', 0.58 for 'zinb' in test_kernel_elements_one_per_sample, at most
1.5 for a gradient in test_kernel_matches_float64.  Per-sample sums: `close` of tests/test_pointwise.py
at 1e-5; step tolerances: the 1e-4 bars of tests/parity_util.py."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

from odin_ai_amd._lib import OdinError
from odin_ai_amd.engine import VAEEngine
from tests import nb_util as nb
from tests.engine_util import Recorder, dense_spec, launch_record
from tests.parity_util import relerr
from tests.test_latent_regularizers import _adam_ref
from tests.test_pointwise import close
from tests.test_vamprior import PLAIN_STEP_CALLS

F64 = torch.float64
U = 2.0 ** -24
CAP = 32.0
MODES = [0, 1]
IDS = ['nb', 'zinb']


def sync(bk):
  if bk.dev.type == 'cuda':
    torch.cuda.synchronize()


def f32(a):
  return np.asarray(a, np.float64).astype(np.float32).astype(np.float64)


# ---- 1. the restatement (CPU) -------------------------------------------------------------------------------------------
def _cpu_inputs(n=4000, zi=True, seed=0):
  p, x = nb.draw(np.random.default_rng(seed), (n, 1), zi)
  return tuple(torch.tensor(v[:, 0]) for v in np.split(p, 3 if zi else 2, -1)), torch.tensor(x[:, 0])


def test_restatement_matches_torch_distributions():
  (a, l, _), x = _cpu_inputs()
  d = torch.distributions.NegativeBinomial(total_count=torch.exp(a), logits=l)
  err = float((nb.nb_log_prob(a, l, x) - d.log_prob(x)).abs().max())
  print(f'log_prob: {err:.2e}')
  assert err <= 1e-9
  assert float((torch.exp(a + l) - d.mean).abs().max() / d.mean.abs().max()) <= 1e-12


def test_closed_form_gradients_match_autograd():
  (a, l, pi), x = _cpu_inputs(seed=1)
  a, l, pi = (t.clone().requires_grad_(True) for t in (a, l, pi))
  for got, ref in ((nb.nb_grads(a, l, x), torch.autograd.grad(nb.nb_log_prob(a, l, x).sum(), (a, l))),
                   (nb.zinb_grads(a, l, pi, x), torch.autograd.grad(nb.zinb_log_prob(a, l, pi, x).sum(), (a, l, pi)))):
    for g, r in zip(got, ref):
      err = float((g - r).detach().abs().max() / max(1.0, float(r.abs().max())))
      assert err <= 1e-9, err


def test_zinb_is_the_mixture_it_restates():
  (a, l, pi), x = _cpu_inputs(seed=2)
  llk = nb.nb_log_prob(a, l, x)
  pos = x > 1e-8
  want = torch.where(pos, torch.nn.functional.logsigmoid(-pi) + llk,
                     torch.log(torch.sigmoid(pi) + torch.sigmoid(-pi) * torch.exp(llk)))
  got = nb.zinb_log_prob(a, l, pi, x)
  assert float((got - want).abs().max()) <= 1e-9
  assert int(pos.sum()) > 100 and int((~pos).sum()) > 100


@pytest.mark.parametrize('a,l', [(0.0, 0.0), (1.5, -1.0), (-2.0, 1.0), (3.0, -2.5), (-6.0, 2.0)])
def test_probabilities_sum_to_one(a, l):
  x = torch.arange(0, 2001, dtype=F64)
  at, lt = torch.full_like(x, a), torch.full_like(x, l)
  assert math.exp(a + l) < 30
  assert abs(float(torch.exp(nb.nb_log_prob(at, lt, x)).sum()) - 1.0) <= 1e-9
  pi = torch.full_like(x, 0.7)
  assert abs(float(torch.exp(nb.zinb_log_prob(at, lt, pi, x)).sum()) - 1.0) <= 1e-9


def _ratio(err, mag):
  return np.abs(err) / (U * np.maximum(1.0, mag))


def test_literal_float32_formula_misses_the_bound():
  """why the kernel forms lgamma(r + x) - lgamma(r) as a difference: the same elements through the literal formula in
  float32 are more than 1000 units off, against the cap of 32"""
  (a, l), x = _cpu_inputs(n=20000, zi=False, seed=3)
  a32, l32, x32 = (t.to(torch.float32) for t in (a, l, x))
  r = torch.exp(a32)
  sp = torch.nn.functional.softplus
  lit = torch.lgamma(r + x32) - torch.lgamma(r) - torch.lgamma(1 + x32) - r * sp(l32) - x32 * sp(-l32)
  ref = nb.nb_log_prob(a, l, x)
  worst = _ratio((lit.to(F64) - ref).numpy(), nb.magnitudes(a, l, x)['M'].numpy()).max()
  print(f'literal float32: {worst:.0f} units')
  assert worst > 1000.0


# ---- 2. the kernel against the restatement ------------------------------------------------------------------------------
def kernel_inputs(B, G, zi, seed=1):
  return nb.draw(np.random.default_rng(seed), (B, G), zi)


def run_kernel(bk, params, x, zi, word=True, scale=None):
  """-> (parts [B, n_part], dparams [B, P G], the range word or None)"""
  L, T = bk.L, bk.T
  B, G = x.shape
  npart, dry = C.c_int(0), C.c_int(0)
  L.odin_elbo_nb_fwd_bwd(None, None, None, None, None, B, G, zi, C.byref(dry), None, None)
  tp, tx, sc = T(params), T(x), T([1.0 / B if scale is None else scale])
  part, dp = bk.full((B * dry.value,), float('nan')), bk.full(params.shape, float('nan'))
  w = bk.zeros(2048, dtype=torch.int32) if word else None
  L.odin_elbo_nb_fwd_bwd(tp.data_ptr(), tx.data_ptr(), part.data_ptr(), dp.data_ptr(), sc.data_ptr(), B, G, zi,
                         C.byref(npart), None if w is None else w.data_ptr(), None)
  sync(bk)
  assert npart.value == dry.value == (G + 255) // 256   # the dry run reports what the real run uses
  return part.reshape(B, -1), dp, w


def reference(params, x, zi):
  """-> (elementwise log p, the gradient planes, the magnitudes) in float64"""
  pl = nb.split(nb.t64(params), 3 if zi else 2)
  xt = nb.t64(x)
  lp = nb.zinb_log_prob(*pl, xt) if zi else nb.nb_log_prob(*pl, xt)
  g = nb.zinb_grads(*pl, xt) if zi else nb.nb_grads(*pl, xt)
  mag = {k: v.numpy() for k, v in nb.magnitudes(pl[0], pl[1], xt, pl[2] if zi else None).items()}
  return lp.numpy(), [t.numpy() for t in g], mag


def check_gradients(dp, B, G, g, mag, x, zi, scale=None):
  """every element of dparams / scale against the closed forms, in units of its own term magnitude"""
  got = dp.cpu().numpy().astype(np.float64) * (B if scale is None else 1.0 / scale)
  zero = zi and (x <= 1e-8)
  wide = np.where(zero, np.maximum(1.0, mag['M']), 1.0)    # (ZINB at x = 0: the gradients carry sigmoid(t1))
  worst = {}
  for p, (name, m) in enumerate([('a', mag['Mg']), ('l', mag['Ml'])] + ([('pi', np.zeros_like(mag['M']))] if zi else [])):
    rt = _ratio(got[:, p * G:(p + 1) * G] + g[p], m) / wide   # (dparams = -scale * gradient)
    worst[name] = float(rt.max())
  print('gradient ratios', worst)
  assert max(worst.values()) <= CAP, worst
  return worst


# (1, 1) | fewer genes than a workgroup | one gene group past a chunk edge | cortex: 8-byte aligned planes | pbmc: 4-byte
@pytest.mark.parametrize('zi', MODES, ids=IDS)
@pytest.mark.parametrize('B,G', [(1, 1), (3, 21), (2, 1028), (3, 558), (2, 2019)])
def test_kernel_matches_float64(bk, B, G, zi):
  params, x = kernel_inputs(B, G, zi)
  part, dp, w = run_kernel(bk, params, x, zi)
  lp, g, mag = reference(params, x, zi)
  got = part.cpu().numpy().astype(np.float64)
  assert np.isfinite(got).all() and bool(torch.isfinite(dp).all())
  close(got.sum(1), lp.sum(1), 1e-5)
  check_gradients(dp, B, G, g, mag, x, zi)
  assert float(w.view(torch.float32).max()) == float(dp.abs().max())


HAND = [(9, 5, 3), (9, 3000, 2900), (20, 5, 3), (30, 1, 0), (-20, 1, 1), (-20, 1, 0), (0, 1, 0), (0, 1, 1.5), (7, 3000, 0),
        (-30, 1, 2), (30, 1e-2, 0), (2.0794415, 3, 4)]   # (the last: r one float32 step off the lifting threshold 8)


@pytest.mark.parametrize('zi', MODES, ids=IDS)
def test_kernel_elements_one_per_sample(bk, zi):
  """G = 1: every element is a sample of its own and its log-likelihood is visible.  The hand-placed (a, mu, x), then
  2000 elements of the random recipe.  This is the test a kernel that subtracts two lgammas fails."""
  rng = np.random.default_rng(5)
  hp = np.array([[a, math.log(mu) - a] for a, mu, _ in HAND])
  hx = np.array([[x] for _, _, x in HAND], np.float64)
  rp, rx = nb.draw(rng, (2000, 1), zi)
  if zi:
    hp = np.concatenate([hp, np.resize([0.0, -3.0, 3.0, 8.0, -8.0], len(HAND))[:, None]], 1)
  params, x = f32(np.concatenate([hp, rp])), f32(np.concatenate([hx, rx]))
  B = x.shape[0]
  part, dp, w = run_kernel(bk, params, x, zi, scale=0.5)
  assert part.shape == (B, 1)
  lp, g, mag = reference(params, x, zi)
  got = part.cpu().numpy().astype(np.float64)[:, 0]
  assert np.isfinite(got).all() and bool(torch.isfinite(dp).all())
  rt = _ratio(got - lp[:, 0], mag['Mz' if zi else 'M'][:, 0])
  k = int(rt.argmax())
  print(f'worst log-likelihood ratio {rt.max():.2f} at (a, l, x) = ({params[k, 0]}, {params[k, 1]}, {x[k, 0]})')
  assert rt.max() <= CAP, (float(rt.max()), params[k].tolist(), float(x[k, 0]))
  assert float(w.view(torch.float32).max()) == float(dp.abs().max())
  if not zi:
    # x = 0: the lgamma and psi differences are exactly 0 -- llk = -r softplus(l), d/da = the same, to 4 ulp
    z = x[:, 0] == 0
    assert z.sum() > 100
    a64, l64 = torch.tensor(params[z, 0]), torch.tensor(params[z, 1])
    want = -(torch.exp(a64) * torch.nn.functional.softplus(l64)).numpy()
    da = dp.cpu().numpy().astype(np.float64)[z, 0] / -0.5
    assert (np.abs(da - want) <= 4 * U * np.abs(want)).all()
    assert (np.abs(got[z] - want) <= 4 * U * np.abs(want)).all()


def test_kernel_refuses_bad_sizes_and_touches_nothing(bk):
  L = bk.L
  tp, tx, sc = bk.zeros(24), bk.zeros(8), bk.full((1,), 0.5)
  part, dp, w = bk.full((8,), 7.0), bk.full((24,), 7.0), bk.zeros(2048, dtype=torch.int32)
  npart = C.c_int(-5)
  for B, G, zi in ((0, 8, 0), (-1, 8, 1), (2, 0, 0), (2, -4, 1), (1, (1 << 28) + 1, 0), (1, 8, 2), (1, 8, -1),
                   (1 << 30, 1024, 0)):
    with pytest.raises(OdinError, match='rc=-2'):
      L.odin_elbo_nb_fwd_bwd(tp.data_ptr(), tx.data_ptr(), part.data_ptr(), dp.data_ptr(), sc.data_ptr(), B, G, zi,
                             C.byref(npart), w.data_ptr(), None)
  for B, G in ((0, 4), (2, 0), (-1, -1), (1, (1 << 28) + 1)):
    with pytest.raises(OdinError, match='rc=-2'):
      L.odin_lognorm_fwd(tx.data_ptr(), part.data_ptr(), B, G, w.data_ptr(), None)
  sync(bk)
  assert npart.value == -5 and bool((part == 7.0).all()) and bool((dp == 7.0).all()) and bool((w == 0).all())


@pytest.mark.parametrize('zi', MODES, ids=IDS)
def test_kernel_is_bit_reproducible_and_feeds_elbo_finalize(bk, zi):
  L, T = bk.L, bk.T
  B, G = 3, 558
  params, x = kernel_inputs(B, G, zi)
  a, b = run_kernel(bk, params, x, zi), run_kernel(bk, params, x, zi)
  assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and torch.equal(a[2], b[2])
  part = a[0]
  llk_ref = reference(params, x, zi)[0].sum(1)
  kl = np.random.default_rng(2).random(B) * 5
  tkl, hyper, ttc = T(kl), T([4.0, 0.5]), T([0.5])
  llk, out = bk.zeros(B), bk.zeros(4)
  L.odin_elbo_finalize(part.data_ptr(), part.shape[1], tkl.data_ptr(), hyper.data_ptr(), ttc.data_ptr(), llk.data_ptr(),
                       out.data_ptr(), B, None)
  sync(bk)
  close(llk.cpu().numpy(), llk_ref, 1e-5)
  loss = -(llk_ref.mean() - 4.0 * kl.mean() - 0.25)
  close(out.cpu().numpy(), [loss, llk_ref.mean(), 4.0 * kl.mean(), 0.25], 1e-5)


# ---- 3. LogNorm ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('B,G', [(1, 1), (3, 558), (2, 2019)])
def test_lognorm(bk, B, G):
  L, T = bk.L, bk.T
  rng = np.random.default_rng(6)
  x = rng.negative_binomial(2.0, 0.1, (B, G)).astype(np.float64)
  x[0] = 0.0                                   # a row of zeros gives zeros
  if B > 1:
    x[1] = x[1] * (1e6 / max(1.0, x[1].sum()))   # a row with total 1e6
    assert abs(f32(x[1]).sum() - 1e6) < 10
  if B == 1:
    x[0, 0] = 7.0
  x = f32(x)
  tx, y, w = T(x), bk.full((B, G), float('nan')), bk.zeros(2048, dtype=torch.int32)
  L.odin_lognorm_fwd(tx.data_ptr(), y.data_ptr(), B, G, w.data_ptr(), None)
  y2 = bk.full((B, G), float('nan'))
  L.odin_lognorm_fwd(tx.data_ptr(), y2.data_ptr(), B, G, None, None)
  sync(bk)
  want = nb.lognorm(nb.t64(x)).numpy()
  close(y.cpu().numpy(), want)
  assert torch.equal(y, y2)
  if B > 1:
    assert bool((y[0] == 0).all())
  amax = float(w.view(torch.float32).max())
  # (y is a float32: at most log1p(1e4) rounded to float32)
  assert amax == float(y.abs().max()) and amax <= float(np.float32(math.log1p(1e4)))


# ---- 4. whole training steps against float64 autograd -------------------------------------------------------------------
def gene_spec(G, units, P, zdim=4):
  """[lognorm, dense u, dense u] -> z -> [dense u, dense u, dense P G]"""
  enc = [('lognorm',), ('dense', units, 'elu'), ('dense', units, 'elu')]
  dec = [('dense', units, 'elu'), ('dense', units, 'elu'), ('dense', P * G, 'linear')]
  return enc, dec, (G,), zdim


def init_params(eng, seed=5):
  """glorot-sized weights; the last layer's bias puts the planes at a = 1, l = 0.5 (pi = 0): a mean of a few counts"""
  rng = np.random.default_rng(seed)
  P = {}
  for key, shp, _ in eng.layout.entries:
    if key[-1] == 'w':
      P[key] = f32(rng.standard_normal(shp) * math.sqrt(2.0 / (shp[0] + shp[1])))
    else:
      P[key] = f32(rng.standard_normal(shp) * 0.05)
  last = max(k[1] for k in P if k[0] == 'dec')
  G = eng.n_per
  P[('dec', last, 'b')][:G] += 1.0
  P[('dec', last, 'b')][G:2 * G] += 0.5
  return P


def counts(rng, B, G):
  x = rng.negative_binomial(2.0, 0.25, (B, G)).astype(np.float32)
  x[rng.random((B, G)) < 0.3] = 0.0
  return x


def step_case(bk, spec, B, obs, calls=None, **kw):
  enc, dec, in_shape, D = spec
  lib = bk.L if calls is None else Recorder(bk.L, calls)
  eng = VAEEngine(enc, dec, in_shape, D, B, bk.dev, lib=lib, observation=obs, **kw)
  P = init_params(eng)
  eng.load_params(P)
  rng = np.random.default_rng(7)
  return eng, P, counts(rng, B, in_shape[0]), rng.standard_normal((B, D)).astype(np.float32)


@pytest.mark.parametrize('obs', IDS)
@pytest.mark.parametrize('G,units', [(21, 32), (558, 256)], ids=['g21', 'cortex'])
def test_three_steps_follow_float64_autograd(bk, G, units, obs):
  zi = obs == 'zinb'
  spec, lr, beta, tol, B = gene_spec(G, units, 3 if zi else 2), 1e-3, 2.0, 1e-4, 4
  calls = []
  eng, P, x, eps = step_case(bk, spec, B, obs, calls)
  assert eng.lognorm and not eng.gauss_head and not eng.fused_tail and not eng.chain_tail
  ref = nb.CountRef(spec[0], spec[1], spec[3], beta, zi)
  M = {k: np.zeros_like(v) for k, v in P.items()}
  V = {k: np.zeros_like(v) for k, v in P.items()}
  xt, et = bk.T(x), bk.T(eps)
  for t in (1, 2, 3):
    f, Gr = ref.loss_and_grads(P, x, eps)
    eng.step_count = t
    eng.set_hyper(lr=lr, beta=beta)
    calls.clear()
    eng.forward(xt, et)
    eng.backward()
    sync(bk)
    assert calls.count('odin_elbo_nb_fwd_bwd') == 1 and calls.count('odin_lognorm_fwd') == 1
    assert calls.index('odin_lognorm_fwd') == 0
    close(eng.x_ln.cpu().numpy(), nb.lognorm(nb.t64(x)).numpy())
    rep = dict(h_d=relerr(eng.dec.outs[-1].cpu().numpy().reshape(f['h_d'].shape), f['h_d']),
               llk=relerr(eng.llk.cpu().numpy(), f['llk']),
               kl=np.abs(eng.kl.cpu().numpy() - f['kl']).max() / max(1.0, np.abs(f['kl']).max()),
               loss=abs(float(eng.out4[0]) - f['loss']) / max(1.0, abs(f['loss'])))
    gv = {k: v.cpu().numpy() for k, v in eng.grad_views().items()}
    assert set(gv) == set(Gr)
    for k in Gr:
      rep['grad' + str(k)] = relerr(gv[k], Gr[k])
    for k, v in rep.items():
      assert v <= tol, (t, k, v)
    eng.adam()
    _adam_ref(P, Gr, M, V, t, lr)
    pv = {k: v.cpu().numpy() for k, v in eng.param_views().items()}
    for k in P:
      # (parity_util's bars: 1e-4 where the gradient is well conditioned, the mean error below 0.5 % of the step size)
      d = np.abs(pv[k] - P[k])
      good = np.abs(Gr[k]) > 1e-3 * np.abs(Gr[k]).max()
      assert d[good].max() <= tol, (t, 'param', k, float(d[good].max()))
      assert d.mean() <= 5e-3 * lr, (t, 'param-mean', k, float(d.mean()))
    eng.load_params(P)   # continue from the reference's parameters: errors do not compound in the check


# ---- 5. launch lists ----------------------------------------------------------------------------------------------------
def flat_dense_spec(P):
  """tests/engine_util.dense_spec over 64 flat genes, with and without LogNorm"""
  enc, dec, _, D = dense_spec()
  return [l for l in enc if l[0] != 'flatten'], dec[:-2] + [('dense', 64 * P, 'linear')], (64,), D


@pytest.mark.parametrize('obs', IDS)
def test_train_step_call_list(bk, obs):
  """the dense Bernoulli step's list with the observation kernel exchanged and odin_lognorm_fwd added in front"""
  from tests.engine_util import case_data
  calls = []
  eng = VAEEngine(*dense_spec(), 4, bk.dev, lib=Recorder(bk.L, calls))
  x, eps = case_data(bk.dev, dense_spec())
  for _ in range(2):
    calls.clear()
    eng.train_step(x, eps, lr=1e-3, beta=2.0)
  bern = list(calls)
  assert bern.count('odin_elbo_bernoulli_fwd_bwd_ranged') == 1
  enc, dec, shp, D = flat_dense_spec(3 if obs == 'zinb' else 2)
  calls2 = []
  eng2 = VAEEngine([('lognorm',)] + enc, dec, shp, D, 4, bk.dev, lib=Recorder(bk.L, calls2), observation=obs)
  eng2.load_params(init_params(eng2))
  xc = bk.T(counts(np.random.default_rng(1), 4, 64))
  for _ in range(2):
    calls2.clear()
    out = eng2.train_step(xc, eps, lr=1e-3, beta=2.0)
  sync(bk)
  assert bool(torch.isfinite(out).all()) and eng2._bern_keeps_top and 'odin_absmax' not in calls2
  want = ['odin_lognorm_fwd'] + ['odin_elbo_nb_fwd_bwd' if c == 'odin_elbo_bernoulli_fwd_bwd_ranged' else c for c in bern]
  assert calls2 == want
  # without LogNorm: no such launch
  calls3 = []
  eng3 = VAEEngine(enc, dec, shp, D, 4, bk.dev, lib=Recorder(bk.L, calls3), observation=obs)
  eng3.load_params(init_params(eng3))
  for _ in range(2):
    calls3.clear()
    eng3.train_step(xc, eps, lr=1e-3, beta=2.0)
  assert calls3 == want[1:]
  with pytest.raises(ValueError, match='lognorm'):
    VAEEngine(enc + [('lognorm',)], dec, shp, D, 4, bk.dev, lib=bk.L, observation=obs)
  with pytest.raises(ValueError, match='flat'):
    VAEEngine(*dense_spec(), 4, bk.dev, lib=bk.L, observation=obs)


def test_plain_bernoulli_call_list_is_unchanged(bk):
  eng, c1 = launch_record(bk)
  assert c1 == PLAIN_STEP_CALLS and eng.observation == 'bernoulli' and not eng.lognorm
  assert 'odin_elbo_nb_fwd_bwd' not in c1 and 'odin_lognorm_fwd' not in c1


@pytest.mark.gpu
@pytest.mark.parametrize('obs', IDS)
def test_graph_replay_equals_eager_and_sees_the_beta_schedule(obs):
  from tests.test_latent_regularizers import _Hip
  bk = _Hip()
  spec = gene_spec(21, 32, 3 if obs == 'zinb' else 2)
  res = []
  for use_graph in (False, True):
    eng, P, x, eps = step_case(bk, spec, 4, obs)
    xt, et = bk.T(x), bk.T(eps)
    outs = [eng.train_step(xt, et, lr=1e-3, beta=b, use_graph=use_graph).clone() for b in (0.5, 1.0, 2.0, 4.0)]
    sync(bk)
    res.append([eng.params.clone(), torch.stack(outs), eng.dp.clone(), eng.llk.clone()])
  for a, b in zip(res[0], res[1]):
    assert torch.equal(a, b)
  assert bool(torch.isfinite(res[0][1]).all()) and len(set(res[0][1][:, 2].tolist())) == 4
  # a beta change between two replays is seen: the KL term scales, the likelihood does not
  eng, P, x, eps = step_case(bk, spec, 4, obs)
  xt, et = bk.T(x), bk.T(eps)
  o1 = eng.train_step(xt, et, lr=0.0, beta=1.0, use_graph=True).clone()
  o2 = eng.train_step(xt, et, lr=0.0, beta=3.0, use_graph=True).clone()
  assert float(o1[1]) == float(o2[1]) and abs(float(o2[2]) - 3.0 * float(o1[2])) <= 1e-5 * abs(float(o2[2]))


# ---- 6. data parallel ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('obs', IDS)
def test_data_parallel_two_ranks(bk, obs):
  """two ranks of 4 against one engine of 8, as tests/test_dp_one_device.py: the kernel is elementwise and `scale`
  carries the global batch"""
  from odin_ai_amd.dist import SegmentedGraph, shard_batch
  from tests.test_dp_one_device import POL, STEPS, Hub, Loopback, check
  spec = gene_spec(21, 32, 3 if obs == 'zinb' else 2)
  W = 2

  def data():
    rng = np.random.default_rng(11)
    return bk.T(counts(rng, 8, 21)), bk.T(rng.standard_normal((8, 4)))

  x, eps = data()
  hub = Hub(W)
  engs = []
  for r in range(W):
    eng = VAEEngine(*spec, 8 // W, bk.dev, lib=bk.L, observation=obs, world_size=W, dp_buckets=2)
    eng.load_params(init_params(eng))
    eng.comm = Loopback(hub, r)
    engs.append(eng)
  shards = [(shard_batch(x, r, W), shard_batch(eps, r, W)) for r in range(W)]
  outs = []
  for _ in range(STEPS):
    progs = []
    for eng, (xs, es) in zip(engs, shards):
      eng.step_count += 1
      eng.set_hyper(lr=1e-3, beta=4.0)
      progs.append(SegmentedGraph(bk.dev, eng.step_program(xs, es, POL)).segs)
    kinds = [''.join(k for k, _ in segs) for segs in progs]
    assert kinds == ['kckck'] * W, kinds
    for s in range(len(progs[0])):
      for segs in progs:
        kind, f = segs[s]
        for fn in (f if kind == 'k' else [f]):
          fn()
      assert not hub.slots
    sync(bk)
    outs.append(engs[0].out4.clone())
  eng1 = VAEEngine(*spec, 8, bk.dev, lib=bk.L, observation=obs)
  eng1.load_params(init_params(eng1))
  outs1 = []
  for _ in range(STEPS):
    eng1.step_count += 1
    eng1.set_hyper(lr=1e-3, beta=4.0)
    for _, fn in eng1.step_program(x, eps, POL):
      fn()
    sync(bk)
    outs1.append(eng1.out4.clone())
  assert all(e.observation == obs and e.B == 4 and e.lognorm for e in engs)
  check(engs, eng1, torch.stack(outs), torch.stack(outs1), term=False)


# ---- 7. networks and the model API --------------------------------------------------------------------------------------
def test_get_networks_cortex_and_pbmc():
  from odin_ai_amd.networks import get_networks
  for name, G, P, obs, zdim, u in (('cortex', 558, 2, 'nb', 10, 256), ('pbmc', 2019, 3, 'zinb', 32, 512)):
    nets = get_networks(name, cnn=False)
    o = nets['observation']
    assert (o.posterior, o.event_shape, o.projection, o.name) == (obs, (G,), True, 'mrna')
    assert nets['encoder'].input_shape == (G,) and nets['latents'].event_shape == (zdim,)
    assert nets['encoder'].layers == [('lognorm',)] + [('dense', u, 'elu')] * 3
    assert nets['decoder'].layers == [('dense', u, 'elu')] * 3 + [('dense', P * G, 'linear')]
    with pytest.raises(NotImplementedError, match='Conv1D'):
      get_networks(name, cnn=True)
    for kw in (dict(is_semi_supervised=True), dict(is_hierarchical=True)):
      with pytest.raises(NotImplementedError):
        get_networks(name, cnn=False, **kw)
  assert get_networks('cortex')['observation'].posterior == 'nb'     # (cnn=False is cortex_networks' default)
  with pytest.raises(NotImplementedError, match='Conv1D'):
    get_networks('pbmc')                                            # (cnn=True is pbmc_networks' default)
  nets = get_networks('cortex', log_norm=False, units=(64, 32), zdim=5)
  assert nets['encoder'].layers == [('dense', 64, 'elu'), ('dense', 32, 'elu')] and nets['latents'].event_shape == (5,)


@pytest.mark.parametrize('alias', ['nbshare', 'nbsingle', 'nbd', 'nbdfull', 'zinbd', 'zinbdshare', 'mixnb', 'mixnbd',
                                   'poisson', 'zip'])
def test_other_count_aliases_stay_refused(alias):
  from odin_ai_amd.networks import _observation
  with pytest.raises(ValueError, match='stay refused'):
    _observation((558,), alias)
  for ok, name in (('nb', 'nb'), ('negativebinomial', 'nb'), ('NB', 'nb'), ('zinb', 'zinb')):
    n, o = _observation((558,), ok)
    assert o.posterior == name and n == 558 * (3 if name == 'zinb' else 2)
  with pytest.raises(ValueError, match='flat'):
    _observation((28, 28, 1), 'nb')


def gene_nets(obs, G=21, units=32, zdim=4):
  from odin_ai_amd.networks import RVconf, SequentialNetwork
  enc, dec, shp, D = gene_spec(G, units, 3 if obs == 'zinb' else 2, zdim)
  return dict(encoder=SequentialNetwork(enc, 'encoder', shp), decoder=SequentialNetwork(dec, 'decoder', (D,)),
              observation=RVconf(shp, obs, projection=True, name='mrna'),
              latents=RVconf((D,), 'mvndiag', projection=True, name='latents'))


def gene_batch(seed, B=8, G=21, D=4):
  rng = np.random.default_rng(seed)
  return counts(rng, B, G), rng.standard_normal((B, D)).astype(np.float32)


@pytest.mark.parametrize('obs', IDS)
def test_api_fit_call_and_the_observation(bk, obs):
  from odin_ai_amd.vae import BetaVAE, NegativeBinomialObservation, ZINegativeBinomialObservation
  zi = obs == 'zinb'
  vae = BetaVAE(beta=1.0, device=bk.dev, lib=bk.L, **gene_nets(obs))
  x, eps = gene_batch(2)
  loss0 = float(vae.optimize(x, training=False)[0])
  vae.fit(x, max_iter=8, batch_size=8, learning_rate=1e-2, compile_graph=False)
  loss1 = float(vae.optimize(x, training=False)[0])
  assert vae.step == 8 and np.isfinite(loss1) and loss1 < loss0, (loss0, loss1)
  px, qz = vae(x, eps=eps)
  cls = ZINegativeBinomialObservation if zi else NegativeBinomialObservation
  assert type(px) is cls and px.event_shape == (21,) and px.batch_shape == (8,)
  assert px.total_count.shape == (8, 21) and px.logits.shape == (8, 21)
  p64, x64 = nb.t64(px.params.cpu().numpy()), nb.t64(x)
  close(px.mean().cpu().numpy(), nb.mean(p64, zi).numpy())
  close(px.total_count.cpu().numpy(), torch.exp(nb.split(p64, 3 if zi else 2)[0]).numpy())
  if zi:
    close(px.rate.cpu().numpy(), torch.sigmoid(nb.split(p64, 3)[2]).numpy())
  lp = px.log_prob(torch.as_tensor(x, device=px.logits.device))
  assert lp.shape == (8,)
  close(lp.cpu().numpy(), nb.log_prob_sum(p64, x64, zi).numpy(), 1e-5)
  llk, kl = vae.elbo_components(x, eps=eps)
  assert llk['llk_mrna'].shape == (8,) and kl['kl_latents'].shape == (8,)
  close(llk['llk_mrna'].cpu().numpy(), lp.cpu().numpy(), 1e-5)
  assert np.isfinite(vae.elbo(llk, kl).cpu().numpy()).all()
  with pytest.raises(NotImplementedError):
    px.sample()
  assert isinstance(vae.decode(vae.encode(x, eps=eps)), cls)
  # sample_shape = (n,): n tiled copies of the batch
  vae3 = BetaVAE(beta=1.0, device=bk.dev, lib=bk.L, sample_shape=(3,), **gene_nets(obs))
  llk3, kl3 = vae3.elbo_components(x)
  assert llk3['llk_mrna'].shape == (3, 8) and bool(torch.isfinite(llk3['llk_mrna']).all())
  assert np.isfinite(float(vae3.optimize(x, learning_rate=1e-3)[0]))


@pytest.mark.parametrize('obs', IDS)
def test_marginal_log_prob_matches_float64_logmeanexp(bk, obs):
  from odin_ai_amd.vae import VariationalAutoencoder
  from oracle.torch_ref import TorchVAE, t_seq
  zi = obs == 'zinb'
  D, n, N = 4, 3, 6
  vae = VariationalAutoencoder(device=bk.dev, lib=bk.L, **gene_nets(obs))
  x, _ = gene_batch(3, B=N)
  eps = np.random.default_rng(4).standard_normal((n, N, D)).astype(np.float32)
  llk, lat = vae.marginal_log_prob(x, n_mcmc=n, reduce=None, batch_size=4, eps=eps)
  T = {k: torch.as_tensor(v.cpu().numpy(), dtype=F64) for k, v in vae.trainable_variables.items()}
  x64 = torch.as_tensor(x, dtype=F64)
  h_e = t_seq(vae.encoder.layers, TorchVAE._sub(T, 'enc'), nb.lognorm(x64))
  p = h_e @ T[('lat', 'w')] + T[('lat', 'b')]
  z = p[None, :, :D] + torch.nn.functional.softplus(p[None, :, D:]) * nb.t64(eps)
  h_d = t_seq(vae.decoder.layers, TorchVAE._sub(T, 'dec'), z.reshape(n * N, D)).reshape(n, N, -1)
  lp = nb.log_prob(h_d, x64[None].expand(n, N, 21), zi).sum(-1)
  want = (torch.logsumexp(lp, 0) - math.log(n)).numpy()
  got = llk['mrna'].cpu().numpy()
  assert np.abs(got - want).max() <= 1e-4 * max(1.0, np.abs(want).max())


@pytest.mark.parametrize('fmt', ['npz', 'tf'])
@pytest.mark.parametrize('obs', IDS)
def test_api_save_load_round_trip(bk, tmp_path, fmt, obs):
  from odin_ai_amd.vae import BetaVAE
  vae = BetaVAE(beta=2.0, device=bk.dev, lib=bk.L, **gene_nets(obs))
  x, eps = gene_batch(2)
  vae.optimize(x, learning_rate=1e-2)
  path = str(tmp_path / 'w')
  vae.save_weights(path, save_format=fmt)
  other = BetaVAE(beta=2.0, device=bk.dev, lib=bk.L, seed=3, **gene_nets(obs))
  assert not torch.equal(other.trainable_variables[('lat', 'w')], vae.trainable_variables[('lat', 'w')])
  other.load_weights(path, raise_notfound=True)
  assert other.step == 1
  for k, v in vae.trainable_variables.items():
    assert torch.equal(v, other.trainable_variables[k]), k
  a, b = vae.elbo_components(x, eps=eps), other.elbo_components(x, eps=eps)
  assert torch.equal(a[0]['llk_mrna'], b[0]['llk_mrna']) and torch.equal(a[1]['kl_latents'], b[1]['kl_latents'])


@pytest.mark.parametrize('obs', IDS)
@pytest.mark.parametrize('name', ['vae', 'betavae', 'annealingvae', 'betatcvae', 'factorvae', 'betacapacityvae', 'infovae',
                                  'dipvae', 'vqvae', 'twostagevae'])
def test_every_model_class_takes_the_observation(bk, name, obs):
  from odin_ai_amd.vae import get_vae
  x, _ = gene_batch(2)
  kw = {'factorvae': dict(discriminator_units=(16, 16)), 'twostagevae': dict(stage2_units=(8, 12))}.get(name, {})
  vae = get_vae(name)(device=bk.dev, lib=bk.L, **kw, **gene_nets(obs))
  vae.fit(x, max_iter=2, batch_size=8, learning_rate=1e-3, compile_graph=False)   # (factorvae: 4 + 4 of the 8)
  # (twostagevae: 2 first-stage steps, then stage2_iter_ratio = 4 times as many second-stage ones)
  assert vae.step == (10 if name == 'twostagevae' else 2)
  assert all(eng.observation == obs and eng.lognorm for eng in vae._engines.values())
  loss, _ = vae.optimize(x, training=False)
  assert np.isfinite(float(loss))
  llk, kl = vae.elbo_components(x[:4] if name == 'factorvae' else x)
  assert bool(torch.isfinite(llk['llk_mrna']).all())
  assert all(bool(torch.isfinite(torch.as_tensor(v)).all()) for v in kl.values())


@pytest.mark.parametrize('obs', IDS)
def test_vampriorvae_refuses_counts(bk, obs):
  from odin_ai_amd.vae import VampriorVAE
  with pytest.raises(ValueError, match=r'\[0, 1\]'):
    VampriorVAE(n_components=5, device=bk.dev, lib=bk.L, **gene_nets(obs))
