"""MultitaskVAE / SkiptaskVAE (multitask_vae.py) on both backends of the `bk` fixture: the float64 restatement of
tests/multitask_util.py against torch.distributions, the label-head kernels of label_head.hip against that restatement,
whole labelled steps against float64 autograd, the untouched unlabelled step, graph replay and the model API.

Tolerances are the project's own (tests/test_two_stage.py): 1e-9 for the restatement against torch, 1e-4 of a tensor's
maximum for values and gradients, 2e-4 of a tensor's largest weight for every parameter after three Adam steps; what the
kernels promise bit for bit (canaries, zero rows, a second run, graph replay) exactly."""
import ctypes as C

import numpy as np
import pytest
import torch

from odin_ai_amd._lib import ReduceJob
from odin_ai_amd.engine import VAEEngine
from odin_ai_amd.interpolation import linear
from odin_ai_amd.networks import RVconf, get_networks
from odin_ai_amd.vae import (AnnealingVAE, MultiheadVAE, MultitaskVAE, OneHotCategoricalLabels, SkiptaskVAE, get_vae)
from tests import multitask_util as mu
from tests.engine_util import tiny_nets, tiny_spec

F64 = torch.float64
CANARY = -12345.5


def sync(bk):
  if bk.dev.type == 'cuda':
    torch.cuda.synchronize()


def ptr(t):
  return None if t is None else t.data_ptr()


# ---- 1. the restatement against torch ---------------------------------------------------------------------------------------
@pytest.mark.parametrize('soft', [False, True])
@pytest.mark.parametrize('D', [1, 3, 10])
def test_restatement_matches_torch(D, soft):
  from torch.distributions import OneHotCategorical
  K, B = 7, 6
  p, eps, W, b, y = (mu.t64(a) for a in mu.head_case(B, B, D, K, 50 + D, soft=soft))
  loc, raw = p[:, :D].clone().requires_grad_(True), p[:, D:].clone().requires_grad_(True)
  W, b = W.clone().requires_grad_(True), b.clone().requires_grad_(True)
  logits = mu.label_logits(loc, raw, eps, W, b)
  got = mu.label_log_prob(logits, y)
  # TFP's _log_prob is linear in y; torch's takes the argmax of its argument, so a soft label is weighed out of torch's
  # values at the K one-hot vectors (for a one-hot label that is torch's own log_prob(y))
  dist = OneHotCategorical(logits=logits)
  basis = torch.stack([dist.log_prob(torch.eye(K, dtype=F64)[k].expand(B, K)) for k in range(K)], -1)
  want = (y * basis).sum(-1)
  if not soft:
    assert torch.allclose(want, dist.log_prob(y), rtol=0, atol=1e-12)
  assert torch.allclose(got, want, rtol=0, atol=1e-9)
  leaves = (loc, raw, W, b)
  g_got = torch.autograd.grad(got.sum(), leaves, retain_graph=True)
  # an independent route to the same gradients: the closed forms of label_head.hip's header
  sm = torch.softmax(logits.detach(), -1)
  g = y - sm * y.sum(-1, keepdim=True)
  dz = g @ W.detach().T
  zp = (loc + torch.nn.functional.softplus(raw) * eps).detach()
  want_g = (dz, dz * eps * torch.sigmoid(raw.detach()), zp.T @ g, g.sum(0))
  for a, w in zip(g_got, want_g):
    assert torch.allclose(a, w, rtol=0, atol=1e-9)


# ---- 2. the kernels against the restatement ---------------------------------------------------------------------------------
def shifted(bk, a, shift):
  """the array on the device, `shift` floats behind a 16-byte boundary"""
  if not shift:
    return bk.T(a)
  buf = bk.zeros(a.size + 4)
  v = buf[shift:shift + a.size].view(a.shape)
  v.copy_(bk.T(a))
  assert v.data_ptr() % 16 == 4 * shift
  return v


def run_head(bk, p, eps, W, b, y, c, row0, pad=2, shift=0, want_logits=True):
  """one fused launch -> dict of numpy outputs (each with `pad` canary rows behind it), the slab's row count and the
  reduced (dW | db)"""
  B, D = p.shape[0], p.shape[1] // 2
  Bs, K = y.shape
  pt, et, Wt, bt, yt = (shifted(bk, a, shift) for a in (p, eps, W, b, y))
  ct = bk.T(np.array([c], np.float32))
  rows = C.c_int(0)
  bk.L.odin_label_head_fwd_bwd(None, None, None, None, None, None, None, None, None, None, None, None, C.byref(rows), B,
                               row0, Bs, D, K, None)
  assert 1 <= rows.value <= 32
  n = D * K + K
  slab = bk.full((rows.value + 1, n), CANARY)
  logits = bk.full((Bs + pad, K), CANARY) if want_logits else None
  llk = bk.full((Bs + pad,), CANARY)
  value = bk.full((2 + pad,), CANARY)
  value[:2] = 0.0
  dloc, dscale = bk.full((B + pad, D), CANARY), bk.full((B + pad, D), CANARY)
  got = C.c_int(0)
  bk.L.odin_label_head_fwd_bwd(ptr(pt), ptr(et), ptr(Wt), ptr(bt), ptr(yt), ptr(ct), ptr(logits), ptr(llk), ptr(value),
                               ptr(dloc), ptr(dscale), ptr(slab), C.byref(got), B, row0, Bs, D, K, None)
  sync(bk)
  assert got.value == rows.value   # (the dry run's count is the real one)
  red = bk.full((n + pad,), CANARY)
  jobs = (ReduceJob * 1)(ReduceJob(slab.data_ptr(), red.data_ptr(), n, rows.value, n, 0))
  bk.L.odin_slab_reduce(jobs, 1, None)
  sync(bk)
  out = dict(llk=llk, value=value, dloc=dloc, dscale=dscale, slab=slab, red=red)
  if want_logits:
    out['logits'] = logits
  return {k: v.cpu().numpy() for k, v in out.items()}, rows.value


def check_head(o, rows, ref, B, Bs, D, K, row0, pad=2):
  if 'logits' in o:
    mu.close(o['logits'][:Bs], ref['logits'])
    assert (o['logits'][Bs:] == CANARY).all()
  mu.close(o['llk'][:Bs], ref['llk'])
  mu.close(o['value'][0], ref['value'])
  assert o['value'][1].view(np.uint32) == 0 and (o['value'][2:] == CANARY).all()   # (the ticket word is back at zero)
  assert (o['llk'][Bs:] == CANARY).all()
  for k in ('dloc', 'dscale'):
    mu.close(o[k][:B], ref[k])
    assert (o[k][B:] == CANARY).all()
    outside = np.r_[o[k][:row0], o[k][row0 + Bs:B]]
    assert (outside == 0.0).all() and not np.signbit(outside).any()   # (exactly zero)
  assert (o['slab'][rows:] == CANARY).all()
  n = D * K + K
  mu.close(o['red'][:D * K].reshape(D, K), ref['dW'])
  mu.close(o['red'][D * K:n], ref['db'])
  assert (o['red'][n:] == CANARY).all()


HEAD_D = [1, 3, 32, 65, 255]
HEAD_K = [1, 2, 7, 10, 64, 65, 255]
HEAD_BS = [1, 5, 33, 67]


@pytest.mark.parametrize('Bs', HEAD_BS)
@pytest.mark.parametrize('K', HEAD_K)
@pytest.mark.parametrize('D', HEAD_D)
def test_label_head_against_restatement(bk, D, K, Bs):
  B = Bs + 3
  p, eps, W, b, y = mu.head_case(B, Bs, D, K, 1000 * D + 10 * K + Bs, soft=(D + K + Bs) % 2 == 0)
  c = -10.0 / Bs
  for row0 in (0, B - Bs):
    ref = mu.head_ref(p, eps, W, b, y, c, row0)
    o, rows = run_head(bk, p, eps, W, b, y, c, row0)
    check_head(o, rows, ref, B, Bs, D, K, row0)
  o2, _ = run_head(bk, p, eps, W, b, y, c, B - Bs)
  for k in o:   # a second call: the same bits
    assert np.array_equal(o[k].view(np.uint32), o2[k].view(np.uint32)), k


@pytest.mark.parametrize('D,K,Bs', [(3, 7, 5), (32, 10, 33), (65, 65, 67), (255, 2, 5)])
def test_label_head_operands_off_the_16_byte_boundary(bk, D, K, Bs):
  B = 2 * Bs
  p, eps, W, b, y = mu.head_case(B, Bs, D, K, 7 + D + K)
  ref = mu.head_ref(p, eps, W, b, y, 0.5, B - Bs)
  o, rows = run_head(bk, p, eps, W, b, y, 0.5, B - Bs, shift=1)
  check_head(o, rows, ref, B, Bs, D, K, B - Bs)
  o0, _ = run_head(bk, p, eps, W, b, y, 0.5, B - Bs, want_logits=False)   # (the optional output left out)
  for k in o0:
    assert np.array_equal(o[k].view(np.uint32), o0[k].view(np.uint32)), k


def test_label_head_extreme_inputs_stay_finite(bk):
  """logits of magnitude 1e4, raw scales of +-80, an all-zero label row"""
  B, Bs, D, K = 12, 9, 5, 7
  p, eps, W, b, y = mu.head_case(B, Bs, D, K, 11)
  rng = np.random.default_rng(12)
  p[:, D:] = np.where(rng.random((B, D)) < 0.5, -80.0, 80.0).astype(np.float32)
  p[1::2, D:] = rng.standard_normal((B // 2, D)).astype(np.float32)
  ref0 = mu.head_ref(p, eps, W, b, y, 1.0, B - Bs)
  W = (W * (1e4 / np.abs(ref0['logits']).max())).astype(np.float32)
  b = (b * 100).astype(np.float32)
  y[4] = 0.0
  ref = mu.head_ref(p, eps, W, b, y, -10.0 / Bs, B - Bs)
  top = np.sort(ref['logits'], -1)
  assert 9e3 < np.abs(ref['logits']).max() < 1.2e4
  # (a float32 logit of this size carries a few ulps of 1e-3; it moves a probability by at most that times the runner-up's
  # share exp(-gap): below 1e-4 of the largest gradient entry, which is of order one, once every gap exceeds 5)
  assert (top[:, -1] - top[:, -2]).min() > 5.0
  o, rows = run_head(bk, p, eps, W, b, y, -10.0 / Bs, B - Bs)
  assert all(np.isfinite(v[:n]).all() for v, n in ((o['logits'], Bs), (o['llk'], Bs), (o['dloc'], B), (o['dscale'], B),
                                                   (o['red'], D * K + K)))
  check_head(o, rows, ref, B, Bs, D, K, B - Bs)
  assert o['llk'][4] == 0.0 and (o['dloc'][B - Bs + 4] == 0.0).all() and (o['dscale'][B - Bs + 4] == 0.0).all()


BAD = [dict(D=0), dict(D=256), dict(K=0), dict(K=256), dict(Bs=0), dict(row0=-1), dict(row0=4), dict(B=5, row0=0, Bs=6)]


@pytest.mark.parametrize('bad', BAD, ids=lambda d: ','.join(f'{k}={v}' for k, v in d.items()))
def test_label_head_limits(bk, bad):
  """B = 8, row0 = 3, Bs = 5, D = 4, K = 3 with one argument out of range: a negative code, nothing touched"""
  a = dict(B=8, row0=3, Bs=5, D=4, K=3)
  a.update(bad)
  bufs = [bk.full((4096,), CANARY) for _ in range(12)]
  rows = C.c_int(-7)
  fn = bk.L.c.odin_label_head_fwd_bwd   # (the raw entry: the wrapper would raise)
  rc = fn(*[ptr(t) for t in bufs], C.byref(rows), a['B'], a['row0'], a['Bs'], a['D'], a['K'], None)
  sync(bk)
  assert rc < 0 and rows.value == -7
  assert all(bool((t == CANARY).all()) for t in bufs)
  if 'D' in bad or 'K' in bad:
    rc = bk.L.c.odin_label_head_fwd(ptr(bufs[0]), ptr(bufs[1]), ptr(bufs[2]), ptr(bufs[3]), 4, a['D'], a['K'], None)
    sync(bk)
    assert rc < 0 and bool((bufs[3] == CANARY).all())
  with pytest.raises(Exception, match='label_head'):
    bk.L.odin_label_head_fwd_bwd(*[ptr(t) for t in bufs], C.byref(rows), a['B'], a['row0'], a['Bs'], a['D'], a['K'], None)


@pytest.mark.parametrize('D,K,n', [(1, 1, 1), (3, 7, 5), (32, 10, 33), (65, 255, 6), (255, 65, 9)])
def test_label_head_fwd_matches_the_fused_launch(bk, D, K, n):
  p, eps, W, b, y = mu.head_case(n, n, D, K, 3 * D + K)
  o, _ = run_head(bk, p, eps, W, b, y, 1.0, 0)
  zp = (mu.t64(p[:, :D]) + mu.softplus(mu.t64(p[:, D:])) * mu.t64(eps)).numpy().astype(np.float32)
  out = bk.full((n + 2, K), CANARY)
  zt, Wt, bt = bk.T(zp), bk.T(W), bk.T(b)
  bk.L.odin_label_head_fwd(ptr(zt), ptr(Wt), ptr(bt), ptr(out), n, D, K, None)
  sync(bk)
  out = out.cpu().numpy()
  mu.close(out[:n], o['logits'][:n])
  mu.close(out[:n], (mu.t64(zp) @ mu.t64(W) + mu.t64(b)).numpy())
  assert (out[n:] == CANARY).all()


# ---- 3. whole steps against float64 autograd --------------------------------------------------------------------------------
VMIN, VMAX, STEPS = 0.3, 1.0, 5   # the annealing schedule of the step tests: beta far from zero in the first steps


def gene_nets(K):
  from tests.test_count_observations import gene_nets as g
  return g('nb'), RVconf(K, 'onehot', projection=True, name='celltype')


def image_nets(K):
  return tiny_nets(), RVconf(K, 'onehot', projection=True, name='digits')


def make_model(bk, kind, K, alpha=10.0, cls=SkiptaskVAE, **kw):
  nets, labels = (gene_nets if kind == 'nb' else image_nets)(K)
  return cls(labels=labels, alpha=alpha, vmin=VMIN, vmax=VMAX, steps=STEPS, device=bk.dev, lib=bk.L, **nets, **kw)


def batch(kind, seed, B=8, D=4, K=3):
  """-> x [B, ...], eps [B, D], y [B / 2, K] one-hot, eps_y [B / 2, D]"""
  rng = np.random.default_rng(seed)
  if kind == 'nb':
    from tests.test_count_observations import gene_batch
    x, eps = gene_batch(seed, B=B, D=D)
  else:
    x = np.clip(rng.random((B, 8, 8, 1)), 1e-6, 1 - 1e-6).astype(np.float32)
    eps = rng.standard_normal((B, D)).astype(np.float32)
  y = np.eye(K, dtype=np.float32)[rng.integers(0, K, B // 2)]
  return x, eps, y, rng.standard_normal((B // 2, D)).astype(np.float32)


def params_of(vae):
  return {k: v.detach().cpu().numpy().astype(np.float64) for k, v in vae.trainable_variables.items()}


def step_ref(vae, kind, kl_form='mc', free_bits=None):
  return mu.StepRef(vae.encoder.layers, vae.decoder.layers, vae.zdim, 'nb' if kind == 'nb' else 'bernoulli', kl_form,
                    free_bits)


def check_step(vae, loss, metrics, f, G, labelled):
  names = vae._names()
  mu.close(float(loss), f['loss'])
  keys = ('uns/llk', 'uns/kl', 'sup/llk', 'sup/kl', 'sup/llk_y') if labelled else ('uns/llk', 'uns/kl')
  assert set(k for k in metrics if not k.startswith('_')) == set(names[:len(keys)])
  for name, k in zip(names, keys):
    mu.close(float(metrics[name]), f[k])
  for k, g in G.items():
    mu.close(metrics['_grad/' + vae.variable_name(k)].cpu().numpy(), g)


def run_steps(bk, kind, K, alpha, kl_form='mc', free_bits=False, clip=False, pattern='LLL'):
  vae = make_model(bk, kind, K, alpha=alpha, analytic=kl_form == 'analytic')
  x, eps, y, eps_y = batch(kind, 5 + K, K=K)
  sched = linear(vmin=VMIN, vmax=VMAX, steps=STEPS)
  P = params_of(vae)
  P0 = {k: v.copy() for k, v in P.items()}
  fb = None
  if free_bits:
    # free bits that clamp some samples and not others: the middle of the widest gap between two KL values of the batch
    from tests.twostage_util import gap_threshold
    probe = step_ref(vae, kind, kl_form)
    T = {k: mu.t64(v) for k, v in P.items()}
    kl0 = probe._elbo_parts(T, mu.t64(x), mu.t64(eps))[1].numpy()
    fb = gap_threshold(kl0, 1e-4) / vae.zdim
    vae.set_elbo_configs(free_bits=fb)
  ref = step_ref(vae, kind, kl_form, fb)
  M, V = ({k: np.zeros_like(v) for k, v in P.items()} for _ in range(2))
  gclip = None
  lr = 1e-3
  for t, kind_t in enumerate(pattern, 1):
    beta = float(sched(t))
    lab = kind_t == 'L'
    f, G = ref.loss_and_grads(P, x, eps, beta, y if lab else None, eps_y if lab else None, alpha)
    if clip and gclip is None:
      # between half and the whole of the restatement's gradient norm: it clips
      gclip = 0.75 * float(np.sqrt(sum((g ** 2).sum() for g in G.values())))
    loss, metrics = vae.optimize((x[:4], x[4:], y) if lab else x, learning_rate=lr, eps=eps, eps_y=eps_y if lab else None,
                                 global_clipnorm=gclip, track_gradients=True)
    sync(bk)
    assert vae.step == t and abs(vae.beta - beta) < 1e-12
    check_step(vae, loss, metrics, f, G, lab)
    mu.adam_ref(P, G, M, V, t, lr, clip=gclip)
  got = params_of(vae)
  for k in P:
    mu.close(got[k], P[k], tol=2e-4)
  return vae, P0, got


@pytest.mark.parametrize('kl_form,free_bits', [('mc', False), ('analytic', False), ('mc', True)])
@pytest.mark.parametrize('K', [3, 7])
@pytest.mark.parametrize('kind', ['image', 'nb'])
def test_labelled_steps_against_autograd(bk, kind, K, kl_form, free_bits):
  run_steps(bk, kind, K, 10.0, kl_form, free_bits)


@pytest.mark.parametrize('kind', ['image', 'nb'])
def test_alpha_zero_leaves_the_label_variables(bk, kind):
  vae, P0, got = run_steps(bk, kind, 3, 0.0)
  for k in (('lab', 'w'), ('lab', 'b')):
    assert np.array_equal(got[k], P0[k]), k


@pytest.mark.parametrize('kind', ['image', 'nb'])
def test_global_clipnorm_sees_the_reference_gradient(bk, kind):
  run_steps(bk, kind, 7, 10.0, clip=True)


# ---- 4. no change without labels ----------------------------------------------------------------------------------------------
def test_unlabelled_steps_are_the_annealing_vae_bit_for_bit(bk):
  nets, labels = image_nets(3)
  kw = dict(vmin=VMIN, vmax=VMAX, steps=STEPS, device=bk.dev, lib=bk.L, seed=4)
  a = AnnealingVAE(**kw, **tiny_nets())
  s = SkiptaskVAE(labels=labels, **kw, **nets)
  w0 = {k: v.clone() for k, v in s.trainable_variables.items() if k[0] == 'lab'}
  assert len(w0) == 2 and float(w0[('lab', 'w')].abs().max()) > 0 and float(w0[('lab', 'b')].abs().max()) == 0
  for k, v in a.trainable_variables.items():
    assert torch.equal(v, s.trainable_variables[k]), k   # (a model with labels starts from the same bits)
  for t in range(3):
    x, eps, _, _ = batch('image', 20 + t)
    la, _ = a.optimize(x, learning_rate=1e-3, eps=eps if t < 2 else None)
    ls, ms = s.optimize((x,) if t == 1 else x, learning_rate=1e-3, eps=eps if t < 2 else None)
    sync(bk)
    assert torch.equal(a._engine(8).out4, s._engine(8).out4) and torch.equal(la, ls)
    assert set(ms) == {'uns/llk_image', 'uns/kl_latents'}
  for k, v in a.trainable_variables.items():
    assert torch.equal(v, s.trainable_variables[k]), k
  for k, v in w0.items():
    assert torch.equal(v, s.trainable_variables[k]), k


def test_unlabelled_step_issues_the_launches_of_an_engine_without_labels(bk):
  from tests.engine_util import Recorder, case_data
  x, eps = case_data(bk.dev, tiny_spec(), B=8)
  rec = {}
  for name, kw in (('plain', {}), ('labels', dict(label_units=3))):
    calls = []
    eng = VAEEngine(*tiny_spec(), 8, bk.dev, lib=Recorder(bk.L, calls), **kw)
    for _ in range(2):
      calls.clear()
      eng.train_step(x, eps, lr=1e-3, beta=2.0)
    rec[name] = list(calls)
  assert rec['plain'] == rec['labels'] and 'odin_label_head_fwd_bwd' not in rec['labels']
  calls.clear()
  y = torch.eye(3, device=bk.dev)[[0, 1, 2, 1]].contiguous()
  eng.train_step(x, eps, lr=1e-3, beta=2.0, labels=y)
  assert calls.count('odin_label_head_fwd_bwd') == 1 and calls.count('odin_rng_normal') == 1
  assert len(calls) == len(rec['plain']) + 2


@pytest.mark.parametrize('kind', ['image', 'nb'])
def test_alternating_steps_against_autograd(bk, kind):
  run_steps(bk, kind, 3, 10.0, pattern='ULU')


# ---- 5. graph replay (GPU only) -----------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_graph_replay_matches_the_eager_program_bit_for_bit():
  from odin_ai_amd import _lib
  L, dev = _lib.load(), torch.device('cuda:0')

  class BK:
    pass
  bk = BK()
  bk.L, bk.dev = L, dev
  outs = {}
  for use_graph in (False, True):
    vae = make_model(bk, 'image', 3, seed=9)
    rows = []
    for t, lab in enumerate((False, True, False, True, True)):
      x, eps, y, eps_y = batch('image', 30 + t)
      # (device noise on the last two steps: the graph draws eps and eps_y from the step's Philox streams as eager does)
      fixed = t < 3
      loss, m = vae.optimize((x[:4], x[4:], y) if lab else x, learning_rate=1e-3, eps=eps if fixed else None,
                             eps_y=eps_y if (lab and fixed) else None, use_graph=use_graph)
      eng = vae._engine(8)
      rows.append(torch.cat([eng.out8.clone(), loss.reshape(1), torch.stack([m[k] for k in sorted(m)])]).cpu())
    torch.cuda.synchronize()
    assert not use_graph or len(eng._graphs) >= 3
    outs[use_graph] = (rows, {k: v.clone().cpu() for k, v in vae.trainable_variables.items()}, eng.m.clone().cpu(),
                       eng.v.clone().cpu())
  for a, b in zip(outs[False][0], outs[True][0]):
    assert torch.equal(a, b)
  for k, v in outs[False][1].items():
    assert torch.equal(v, outs[True][1][k]), k
  assert torch.equal(outs[False][2], outs[True][2]) and torch.equal(outs[False][3], outs[True][3])


# ---- 6. the model API -----------------------------------------------------------------------------------------------------------
def test_get_vae_and_networks():
  assert get_vae('skiptaskvae') is SkiptaskVAE and get_vae('multitaskvae') is MultitaskVAE
  assert get_vae('Skiptask_VAE') is SkiptaskVAE
  for ds in ('mnist', 'binarizedmnist', 'fashionmnist'):
    nets = get_networks(ds, is_semi_supervised=True)
    lab = nets['labels']
    assert lab.event_shape == (10,) and lab.posterior == 'onehot' and lab.projection and lab.name == 'digits'
    assert 'labels' not in get_networks(ds)
  assert get_networks('mnist', is_semi_supervised=True, labels_name='clothes')['labels'].name == 'clothes'
  for ds in ('dsprites', 'shapes3d', 'celeba', 'cortex', 'pbmc'):
    with pytest.raises(NotImplementedError):
      get_networks(ds, is_semi_supervised=True)
  with pytest.raises(NotImplementedError):
    get_networks('mnist', is_semi_supervised=True, is_hierarchical=True)


def test_model_refusals(bk):
  nets, labels = image_nets(3)
  kw = dict(device=bk.dev, lib=bk.L, **nets)
  cases = [
      (MultitaskVAE, dict(labels=labels), 'skip_decoder=False'),
      (MultitaskVAE, dict(labels=labels, skip_decoder=False), 'skip_decoder=False'),
      (SkiptaskVAE, dict(labels=labels, encoder_y='tie'), 'encoder_y'),
      (MultitaskVAE, dict(labels=labels, skip_decoder=True, decoder_y=[('dense', 8, 'relu')]), 'decoder_y'),
      (SkiptaskVAE, dict(labels=labels, n_semi_iw=3), 'n_semi_iw'),
      (SkiptaskVAE, dict(labels=labels, sample_shape=(2,)), 'sample_shape'),
      (SkiptaskVAE, dict(labels=labels, sample_shape=2), 'sample_shape'),
      (SkiptaskVAE, dict(labels=RVconf(3, 'categorical', projection=True, name='y')), 'posterior'),
      (SkiptaskVAE, dict(labels=RVconf(3, 'onehot', projection=False, name='y')), 'projection'),
      (SkiptaskVAE, dict(labels=[labels, labels]), 'list of label variables'),
      (MultiheadVAE, dict(labels=labels), 'batch-normalised'),
  ]
  for cls, extra, msg in cases:
    with pytest.raises(NotImplementedError, match=msg):
      cls(**extra, **kw)
  vae = SkiptaskVAE(labels=labels, **kw)
  with pytest.raises(NotImplementedError, match='sample_shape'):
    vae.set_elbo_configs(sample_shape=(3,))
  x, _, y, _ = batch('image', 1)
  with pytest.raises(ValueError, match='equal halves'):
    vae.optimize((x[:4], x[4:7], y[:3]))
  with pytest.raises(ValueError, match='labels'):
    vae.optimize((x[:4], x[4:], y[:, :2]))
  with pytest.raises(ValueError, match='x_u, x_s, y_s'):
    vae.optimize((x[:4], x[4:]))
  with pytest.raises(ValueError, match='outside'):
    vae.optimize((x[:4], x[4:], np.array([0, 1, 2, 3])))
  for posterior in ('mvntril', 'relaxedonehot', 'relaxedbernoulli'):
    bad = dict(nets, latents=RVconf((4,), posterior, projection=True, name='latents'))
    with pytest.raises(ValueError, match='mvndiag'):
      SkiptaskVAE(labels=labels, device=bk.dev, lib=bk.L, **bad)


def test_engine_refusals(bk):
  spec = tiny_spec()
  mk = lambda **kw: VAEEngine(*spec, 4, bk.dev, lib=bk.L, label_units=3, **kw)
  for kw, exc in ((dict(tc='betatc'), ValueError), (dict(latent_reg='mmd'), ValueError),
                  (dict(latent_reg='dip_i'), ValueError), (dict(vamprior_components=4), ValueError),
                  (dict(vq_codes=8), ValueError), (dict(latent_cov='tril'), NotImplementedError),
                  (dict(latent_dist='relaxedonehot'), NotImplementedError),
                  (dict(latent_dist='relaxedbernoulli'), NotImplementedError), (dict(force_dp=True), NotImplementedError)):
    with pytest.raises(exc):
      mk(**kw)
  with pytest.raises(ValueError):
    VAEEngine(*spec, 4, bk.dev, lib=bk.L, label_units=256)
  eng = VAEEngine(*spec, 5, bk.dev, lib=bk.L, label_units=3)
  with pytest.raises(ValueError, match='odd'):
    eng.set_labels(torch.zeros(2, 3, device=bk.dev))


def test_input_forms_call_and_predict_labels(bk):
  vae = make_model(bk, 'image', 3, seed=2)
  x, eps, y, eps_y = batch('image', 3)
  # x, (x,) and integer classes
  l0, _ = vae.optimize(x, training=False, eps=eps)
  l1, _ = vae.optimize((x,), training=False, eps=eps)
  assert torch.equal(l0, l1)
  cls = y.argmax(-1)
  a = vae.optimize((x[:4], x[4:], y), training=False, eps=eps, eps_y=eps_y)
  b = vae.optimize((x[:4], x[4:], cls), training=False, eps=eps, eps_y=eps_y)
  assert torch.equal(a[0], b[0]) and vae.step == 0
  # elbo_components / elbo / train_steps: the reference's loss through the generic VAEStep
  llk, kl = vae.elbo_components((x[:4], x[4:], y), eps=eps, eps_y=eps_y)
  assert set(llk) == {'uns/llk_image', 'sup/llk_image', 'sup/llk_digits'} and set(kl) == {'uns/kl_latents', 'sup/kl_latents'}
  assert llk['uns/llk_image'].shape == (4,) and llk['sup/llk_image'].dim() == 0
  mu.close(float(-vae.elbo(llk, kl).mean()), float(a[0]))
  loss, metrics = next(iter(vae.train_steps((x[:4], x[4:], y), training=False, eps=eps, eps_y=eps_y)))()
  mu.close(float(loss), float(a[0]))
  assert set(metrics) == set(vae._names())
  llk_u, kl_u = vae.elbo_components(x, eps=eps)
  assert set(llk_u) == {'uns/llk_image'} and set(kl_u) == {'uns/kl_latents'} and llk_u['uns/llk_image'].shape == (8,)
  # call
  (px, py), qz = vae(x, eps=eps)
  (px3, py3), qz3 = vae((x[:4], x[4:], y), eps=eps[:4])
  assert px.mean().shape == (8, 8, 8, 1) and isinstance(py, OneHotCategoricalLabels) and py.logits.shape == (8, 3)
  assert qz.mean().shape == (8, 4) and px3.mean().shape == (4, 8, 8, 1) and py3.logits.shape == (4, 3)
  # predict_labels
  py = vae.predict_labels(x, mean=True)
  W, bb = (vae.trainable_variables[k].cpu().to(F64) for k in (('lab', 'w'), ('lab', 'b')))
  want = vae.encode(x).mean().cpu().to(F64) @ W + bb
  mu.close(py.logits.cpu().numpy(), want.numpy())
  assert py.mode().shape == (8, 3) and bool((py.mode().sum(-1) == 1).all())
  assert torch.equal(py.mode().argmax(-1), py.logits.argmax(-1))
  mu.close(py.probs_parameter().cpu().numpy(), torch.softmax(want, -1).numpy())
  assert torch.equal(py.mean(), py.probs_parameter())
  yy = torch.eye(3)[[0, 1, 2, 0, 1, 2, 0, 1]]
  mu.close(py.log_prob(yy).cpu().numpy(), mu.label_log_prob(want, yy.to(F64)).numpy())
  assert py.sample().shape == (8, 3) and py.sample(5).shape == (5, 8, 3)
  z = torch.randn(5, 4)
  mu.close(vae.predict_labels(latents=z).logits.cpu().numpy(), (z.to(F64) @ W + bb).numpy())
  assert vae.predict_labels(latents=vae.encode(x)).logits.shape == (8, 3)   # (a fresh sample of the posterior)


@pytest.mark.parametrize('fmt', ['tf', 'npz'])
def test_checkpoint_round_trip(bk, tmp_path, fmt):
  vae = make_model(bk, 'image', 3, seed=2)
  x, eps, y, eps_y = batch('image', 3)
  for _ in range(2):
    vae.optimize((x[:4], x[4:], y), learning_rate=1e-2, eps=eps, eps_y=eps_y)
  assert vae.variable_name(('lab', 'w')) == 'digits/kernel' and vae.variable_name(('lab', 'b')) == 'digits/bias'
  path = str(tmp_path / 'w')
  vae.save_weights(path, save_format=fmt)
  other = make_model(bk, 'image', 3, seed=5)
  assert not torch.equal(other.trainable_variables[('lab', 'w')], vae.trainable_variables[('lab', 'w')])
  other.load_weights(path, raise_notfound=True)
  assert other.step == 2
  for k, v in vae.trainable_variables.items():
    assert torch.equal(v, other.trainable_variables[k]), k
  slots = lambda m: [t.clone() for _, a, b in m._label_slots() for t in (a, b)]
  assert all(float(t.abs().max()) > 0 for t in slots(vae))
  for a, b in zip(slots(vae), slots(other)):
    assert torch.equal(a, b)
  assert torch.equal(vae.predict_labels(x, mean=True).logits, other.predict_labels(x, mean=True).logits)


def test_fit_over_three_tuples_learns_the_labels(bk):
  """two blobs: class 0 lights the left half of the image, class 1 the right half"""
  rng = np.random.default_rng(8)

  def blobs(n):
    c = rng.integers(0, 2, n)
    x = np.full((n, 8, 8, 1), 0.1, np.float32)
    for i, k in enumerate(c):
      x[i, :, 4 * k:4 * k + 4] = 0.9
    return np.clip(x + 0.05 * rng.standard_normal(x.shape).astype(np.float32), 0.01, 0.99), c

  train = []
  for i in range(44):
    (xu, _), (xs, c) = blobs(4), blobs(4)
    train.append((xu, xs, c))
    if i % 11 == 5:
      train.append(blobs(8)[0])   # (plain arrays in between: unlabelled steps)
  # (Dense layers only: 48 steps stay quick on the simulator)
  from odin_ai_amd.networks import SequentialNetwork
  nets = dict(encoder=SequentialNetwork([('flatten',), ('dense', 16, 'relu')], 'Encoder', (8, 8, 1)),
              decoder=SequentialNetwork([('dense', 16, 'relu'), ('dense', 64, 'linear'), ('reshape', (8, 8, 1))], 'Decoder',
                                        (4,)),
              observation=RVconf((8, 8, 1), 'bernoulli', projection=True, name='image'),
              latents=RVconf((4,), 'mvndiag', projection=True, name='latents'))
  vae = SkiptaskVAE(labels=RVconf(2, 'onehot', projection=True, name='digits'), device=bk.dev, lib=bk.L, seed=3, **nets)
  seen, kinds = [], []

  def on_batch_end():
    m = vae.last_train_metrics
    kinds.append(len(m))
    if 'sup/llk_digits' in m:
      seen.append(float(m['sup/llk_digits']))

  vae.fit(train, max_iter=len(train), learning_rate=5e-3, on_batch_end=on_batch_end, valid=train[:3], valid_freq=1000)
  assert vae.step == 48 and len(seen) == 44 and sorted(set(kinds)) == [2, 5]
  assert np.isfinite(vae.last_valid_loss) and 'sup/llk_digits' in vae.last_valid_metrics
  assert np.mean(seen[-20:]) > np.mean(seen[:20]), (np.mean(seen[:20]), np.mean(seen[-20:]))
