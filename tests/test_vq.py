"""VQVAE (vq.hip, VAEEngine(vq_codes=K), odin_ai_amd.vae.VQVAE) on both backends of the `bk` fixture: the quantiser
kernels against the float64 restatement of tests/vq_util.py, whole training steps against float64 autograd with the
stop_gradient structure written out by hand, the engine's behaviour and the model API.

Tolerances: 1e-4 of a tensor's maximum for values and gradients (the project's parity bound); counts exact; the
moving-average state to 1e-6 relative (the kernel forms it in float64 from the same float32 inputs and rounds once:
6e-8 per stored value, twice for the codebook); near ties of the argmin by the rule of vq_util.check_assignment."""
import math

import numpy as np
import pytest
import torch

from odin_ai_amd._lib import OdinError
from odin_ai_amd.engine import RANGE_WORDS, VAEEngine
from oracle import vae_oracle as vo
from tests.engine_util import launch_record, tiny_spec
from tests.range_audit import RangeAudit
from tests.test_latent_regularizers import _adam_ref, _Hip, api_nets
from tests.test_vamprior import PLAIN_STEP_CALLS
from tests.vq_util import VQRef, assign64, bwd64, check_assignment, ema64, near_ties

I32 = torch.int32


# ---- 1. kernels ---------------------------------------------------------------------------------------------------------
def run_assign(bk, codes, codebook, count=True, word=False):
  N, Cs = codes.shape
  K = codebook.shape[0]
  idx = bk.zeros(N, dtype=I32)
  zq = bk.zeros(N, Cs)
  ws = bk.zeros(bk.L.odin_vq_workspace(N))
  m = bk.zeros(2)
  cnt = bk.zeros(K, dtype=I32) if count else None
  w = bk.zeros(RANGE_WORDS, dtype=I32) if word else None
  ct, et = bk.T(codes), bk.T(codebook)   # (kept alive across the call)
  bk.L.odin_vq_assign(ct.data_ptr(), et.data_ptr(), idx.data_ptr(), zq.data_ptr(), ws.data_ptr(),
                      m.data_ptr(), cnt.data_ptr() if count else None, w.data_ptr() if word else None, N, K, Cs, None)
  if bk.dev.type == 'cuda':
    torch.cuda.synchronize()
  return idx.cpu(), zq.cpu(), m[:1].cpu(), (cnt.cpu() if count else None), (w.cpu() if word else None)


def run_bwd(bk, codes, zq, idx, dzq, codebook, commitment, mode, state=None, decay=0.99, epsilon=1e-5, act=0):
  """mode 'grad' | 'ema' | 'none'; -> (dcodes, dcodebook | None, (counts, means, codebook) | None, range word)"""
  N, Cs = codes.shape
  K = codebook.shape[0]
  dc = bk.zeros(N, Cs)
  cb = bk.T(codebook)
  dcb = bk.zeros(K, Cs) if mode == 'grad' else None
  ec, em = (bk.T(state[0]), bk.T(state[1])) if mode == 'ema' else (None, None)
  w = bk.zeros(RANGE_WORDS, dtype=I32)
  ct, zt, it, dt = bk.T(codes), bk.T(zq), bk.T(idx, I32), bk.T(dzq)   # (kept alive across the call)
  bk.L.odin_vq_bwd(ct.data_ptr(), zt.data_ptr(), it.data_ptr(), dt.data_ptr(),
                   cb.data_ptr(), dc.data_ptr(), dcb.data_ptr() if dcb is not None else None,
                   ec.data_ptr() if ec is not None else None, em.data_ptr() if em is not None else None,
                   float(commitment), float(decay), float(epsilon), act, w.data_ptr(), N, K, Cs, None)
  if bk.dev.type == 'cuda':
    torch.cuda.synchronize()
  st = (ec.cpu().numpy(), em.cpu().numpy(), cb.cpu().numpy()) if mode == 'ema' else None
  return dc.cpu().numpy(), (dcb.cpu().numpy() if dcb is not None else None), st, w.cpu()


def close(got, ref, tol=1e-4):
  got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
  scale = max(float(np.abs(ref).max()), 1e-30)
  err = float(np.abs(got - ref).max())
  assert err <= tol * scale, (err, scale)


def rel_close(got, ref, tol=1e-6):
  got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
  assert (np.abs(got - ref) <= tol * np.abs(ref)).all(), float(np.abs(got - ref).max())


VQ_SIZES = [(24, 5, 4), (256, 64, 128), (2048, 512, 16), (2048, 256, 32), (4096, 1024, 8)]


@pytest.mark.parametrize('N,K,Cs', VQ_SIZES)
def test_vq_kernels_match_float64(bk, N, K, Cs):
  rng = np.random.default_rng(N + K)
  codes = rng.standard_normal((N, Cs)).astype(np.float32)
  codebook = rng.standard_normal((K, Cs)).astype(np.float32)
  idx, zq, m, cnt, w = run_assign(bk, codes, codebook, word=True)
  ridx, rzq, rm, rcnt, dist = assign64(codes, codebook)
  n_ties = check_assignment(idx.numpy(), dist)
  print(f'near ties: {n_ties} of {N}; m {float(m):.8g} vs {rm:.8g}')
  ki = idx.numpy().astype(np.int64)
  # everything below is a function of the assignments: the float64 side takes the kernel's (accepted above)
  assert np.array_equal(zq.numpy(), codebook[ki])
  rm_k = float(((codes.astype(np.float64) - codebook[ki].astype(np.float64)) ** 2).mean())
  assert abs(float(m) - rm_k) <= 1e-4 * rm_k
  assert abs(float(m) - rm) <= 1e-4 * rm
  assert np.array_equal(cnt.numpy(), np.bincount(ki, minlength=K))
  assert float(w.view(torch.float32).max()) == float(np.abs(codebook[ki]).max())
  dzq = rng.standard_normal((N, Cs)).astype(np.float32) * 1e-2
  rdc, rdcb = bwd64(codes, codebook, ki, dzq, 0.25)
  dc, dcb, _, w2 = run_bwd(bk, codes, zq.numpy(), ki, dzq, codebook, 0.25, 'grad')
  close(dc, rdc)
  close(dcb, rdcb)
  assert float(w2.view(torch.float32).max()) == float(np.abs(dc).max())
  counts0 = rng.random(K).astype(np.float32) * 3
  means0 = rng.standard_normal((K, Cs)).astype(np.float32)
  dc2, none, st, _ = run_bwd(bk, codes, zq.numpy(), ki, dzq, codebook, 0.25, 'ema', (counts0, means0))
  assert none is None and np.array_equal(dc2, dc)
  nc, nm, ncb = ema64(codes, ki, counts0, means0, 0.99, 1e-5)
  rel_close(st[0], nc)
  rel_close(st[1], nm)
  rel_close(st[2], ncb)
  dc3, _, _, _ = run_bwd(bk, codes, zq.numpy(), ki, dzq, codebook, 0.25, 'none')
  assert np.array_equal(dc3, dc)


def test_vq_duplicated_rows_smaller_index_wins(bk):
  rng = np.random.default_rng(0)
  codebook = rng.standard_normal((70, 6)).astype(np.float32)
  codebook[[9, 40, 69]] = codebook[3]
  codebook[65] = codebook[64]
  codes = rng.standard_normal((300, 6)).astype(np.float32)
  codes[:50] = codebook[3] + 1e-3 * rng.standard_normal((50, 6)).astype(np.float32)
  codes[50:60] = codebook[64]
  idx, _, _, cnt, _ = run_assign(bk, codes, codebook)
  idx = idx.numpy()
  assert (idx[:50] == 3).all() and (idx[50:60] == 64).all()
  assert not np.isin(idx, [9, 40, 69, 65]).any() and cnt.numpy()[[9, 40, 69, 65]].sum() == 0


def test_vq_codes_equal_to_rows(bk):
  rng = np.random.default_rng(1)
  codebook = rng.standard_normal((33, 20)).astype(np.float32)
  pick = rng.integers(0, 33, 100)
  codes = codebook[pick]
  idx, zq, m, cnt, _ = run_assign(bk, codes, codebook)
  assert np.array_equal(idx.numpy(), pick) and float(m) == 0.0 and np.array_equal(zq.numpy(), codes)
  dzq = rng.standard_normal(codes.shape).astype(np.float32)
  dc, dcb, _, _ = run_bwd(bk, codes, zq.numpy(), pick, dzq, codebook, 0.25, 'grad')
  assert np.array_equal(dc, dzq) and not dcb.any()


def test_vq_single_code_and_unused_code(bk):
  rng = np.random.default_rng(2)
  codes = rng.standard_normal((37, 5)).astype(np.float32)
  one = rng.standard_normal((1, 5)).astype(np.float32)
  idx, zq, m, cnt, _ = run_assign(bk, codes, one)
  assert not idx.numpy().any() and int(cnt[0]) == 37
  assert abs(float(m) - assign64(codes, one)[2]) <= 1e-4 * float(m)
  # a far-away code is used by no row: zero gradient, decay only
  codebook = np.concatenate([rng.standard_normal((4, 5)), np.full((1, 5), 1e3)]).astype(np.float32)
  idx, zq, m, cnt, _ = run_assign(bk, codes, codebook)
  assert int(cnt[4]) == 0
  dzq = np.zeros_like(codes)
  _, dcb, _, _ = run_bwd(bk, codes, zq.numpy(), idx.numpy(), dzq, codebook, 0.25, 'grad')
  assert not dcb[4].any() and dcb[:4].any()
  c0, m0 = np.full(5, 2.0, np.float32), rng.standard_normal((5, 5)).astype(np.float32)
  _, _, st, _ = run_bwd(bk, codes, zq.numpy(), idx.numpy(), dzq, codebook, 0.25, 'ema', (c0, m0), decay=0.9)
  rel_close(st[0][4], 0.9 * 2.0)
  rel_close(st[1][4], 0.9 * m0[4].astype(np.float64))
  rel_close(st[2][4], 0.9 * m0[4].astype(np.float64) / (0.9 * 2.0 + 1e-5))


def test_vq_activation_derivative(bk):
  """act: the derivative of the activation that produced the codes (from its output), as the Dense data gradient"""
  rng = np.random.default_rng(3)
  codes = np.maximum(rng.standard_normal((40, 8)), 0).astype(np.float32)
  codebook = rng.standard_normal((6, 8)).astype(np.float32)
  idx, zq, _, _, _ = run_assign(bk, codes, codebook)
  dzq = rng.standard_normal(codes.shape).astype(np.float32)
  lin, _, _, _ = run_bwd(bk, codes, zq.numpy(), idx.numpy(), dzq, codebook, 0.25, 'none')
  relu, _, _, _ = run_bwd(bk, codes, zq.numpy(), idx.numpy(), dzq, codebook, 0.25, 'none', act=2)
  assert np.array_equal(relu, lin * (codes > 0))


def test_vq_limits_return_their_error_code(bk):
  c = bk.L.c
  buf = bk.zeros(1 << 16)
  p = buf.data_ptr()
  for N, K, Cs in ((65537, 4, 4), (0, 4, 4), (8, 1025, 4), (8, 0, 4), (8, 4, 257), (8, 4, 0), (8, 1024, 32),
                   (8, 128, 256)):
    assert c.odin_vq_assign(p, p, p, p, p, p, None, None, N, K, Cs, None) == -2, (N, K, Cs)
    assert c.odin_vq_bwd(p, p, p, p, p, p, None, None, None, 0.25, 0.99, 1e-5, 0, None, N, K, Cs, None) == -2
  with pytest.raises(OdinError):
    bk.L.odin_vq_assign(p, p, p, p, p, p, None, None, 8, 1024, 32, None)
  # both ways of training the codebook at once, half a moving-average state, an unknown activation
  assert c.odin_vq_bwd(p, p, p, p, p, p, p, p, p, 0.25, 0.99, 1e-5, 0, None, 8, 4, 4, None) == -2
  assert c.odin_vq_bwd(p, p, p, p, p, p, None, p, None, 0.25, 0.99, 1e-5, 0, None, 8, 4, 4, None) == -2
  assert c.odin_vq_bwd(p, p, p, p, p, p, None, None, None, 0.25, 0.99, 1e-5, 3, None, 8, 4, 4, None) == -2
  assert c.odin_vq_assign(p, p, p, p, p + 4, p, None, None, 8, 4, 4, None) == -2   # (workspace alignment)
  run_assign(bk, np.ones((8, 256), np.float32), np.zeros((64, 256), np.float32))   # exactly the 64 KB: accepted


def test_vq_forward_only_and_reproducible(bk):
  rng = np.random.default_rng(4)
  codes = rng.standard_normal((1000, 16)).astype(np.float32)
  codebook = rng.standard_normal((300, 16)).astype(np.float32)
  a = run_assign(bk, codes, codebook)
  b = run_assign(bk, codes, codebook, count=False)
  c = run_assign(bk, codes, codebook)
  for i in range(3):
    assert torch.equal(a[i], b[i]) and torch.equal(a[i], c[i])
  assert torch.equal(a[3], c[3]) and b[3] is None
  dzq = rng.standard_normal(codes.shape).astype(np.float32)
  st0 = (rng.random(300).astype(np.float32), rng.standard_normal((300, 16)).astype(np.float32))
  for mode in ('grad', 'ema'):
    r1 = run_bwd(bk, codes, a[1].numpy(), a[0].numpy(), dzq, codebook, 0.25, mode, st0)
    r2 = run_bwd(bk, codes, a[1].numpy(), a[0].numpy(), dzq, codebook, 0.25, mode, st0)
    assert np.array_equal(r1[0], r2[0])
    if mode == 'grad':
      assert np.array_equal(r1[1], r2[1])
    else:
      assert all(np.array_equal(x, y) for x, y in zip(r1[2], r2[2]))


# ---- 2. whole steps against float64 autograd ----------------------------------------------------------------------------
def dense_spec(maps=1):
  enc = [('flatten',), ('dense', 32, 'relu'), ('dense', 16, 'relu')]
  dec = [('dense', 32, 'relu'), ('dense', 64 * maps, 'linear'), ('reshape', (8, 8, maps))]
  return enc, dec, (8, 8, 1)


def conv_spec(maps=1):
  enc, dec, in_shape, _ = tiny_spec()
  return enc, dec[:-1] + [('conv', maps, 1, 1, 'linear')], in_shape


def init_nets(enc, dec, in_shape, H, seed=5):
  """the networks' parameters through OracleVAE's initialiser (the decoder built on the H-wide input)"""
  P = vo.OracleVAE(enc, dec, in_shape, H, observation='bernoulli').init_params(seed=seed)
  return {k: np.asarray(v, np.float64) for k, v in P.items() if k[0] != 'lat'}


def vq_case(bk, spec, B, K, Cs, obs='bernoulli', ema=False, seed=7, cw=0.25, **engkw):
  enc, dec, in_shape = spec
  rng = np.random.default_rng(seed)
  x = np.clip(rng.random((B,) + tuple(in_shape)), 1e-6, 1 - 1e-6)
  probe = VAEEngine(enc, dec, in_shape, 1, B, bk.dev, lib=bk.L, observation=obs, vq_codes=K, vq_code_size=Cs,
                    vq_commitment=cw, vq_ema=ema, **engkw)
  H = probe.hdim
  P = init_nets(enc, dec, in_shape, H)
  # a codebook among the codes: several codes in use
  cb = (rng.standard_normal((K, Cs or H)) * 0.3).astype(np.float32).astype(np.float64)
  eng = probe
  if ema:
    eng.load_params(P)
    eng.init_codebook(cb)
  else:
    eng.load_params({**P, ('vq', 'codebook'): cb})
  return eng, P, cb, x


def step_vs_autograd(bk, spec, B, K, Cs, obs='bernoulli', ema=False, beta=1.5, tol=1e-4, **engkw):
  eng, P, cb, x = vq_case(bk, spec, B, K, Cs, obs, ema, **engkw)
  eng.step_count = 1
  eng.set_hyper(beta=beta)
  eng.forward(bk.T(x))
  eng.backward()
  if bk.dev.type == 'cuda':
    torch.cuda.synchronize()
  ref = VQRef(spec[0], spec[1], obs, K, Cs, 0.25, ema, beta)
  f0, _ = ref.loss_and_grads(P, cb, x)
  dist = ((f0['codes'][:, None, :] - cb[None]) ** 2).sum(-1)
  ki = eng.vq_idx.cpu().numpy()
  check_assignment(ki, dist)
  f, G = ref.loss_and_grads(P, cb, x, idx=ki)
  out8 = eng.out8.cpu().numpy()
  L = eng.vq_L
  assert len(np.unique(ki)) > 1 or K == 1
  assert abs(out8[0] - f['loss']) <= tol * max(1.0, abs(f['loss'])), (out8[0], f['loss'])
  close(eng.llk.cpu().numpy(), f['llk'], tol)
  assert abs(out8[1] - f['llk'].mean()) <= tol * max(1.0, abs(f['llk'].mean()))
  assert abs(out8[2] - beta * L * math.log(K)) <= tol * max(1.0, f['kl'])
  assert abs(out8[3] - f['extra']) <= tol * max(1e-30, abs(f['extra'])), (out8[3], f['extra'])
  assert abs(out8[4] - f['m']) <= tol * f['m']
  gv = {k: v.cpu().numpy() for k, v in eng.grad_views().items()}
  assert set(gv) == set(G), (sorted(gv), sorted(G))
  for k in G:
    close(gv[k], G[k], tol)
  assert ('vq', 'codebook') in gv or ema
  assert not any(k[0] == 'lat' for k in gv)
  return eng, P, cb, x, ki


STEP_CASES = [('conv', 5, None, 'bernoulli', False), ('conv', 6, 8, 'bernoulli', True),
              ('conv', 7, 8, 'gaussian_softplus1', False), ('conv', 4, None, 'gaussian_softplus1', True),
              ('dense', 9, 4, 'bernoulli', False), ('dense', 5, None, 'gaussian_softplus1', True),
              ('dense', 6, 4, 'bernoulli', True), ('dense', 3, None, 'gaussian_softplus1', False)]


@pytest.mark.parametrize('net,K,Cs,obs,ema', STEP_CASES)
def test_step_matches_float64_autograd(bk, net, K, Cs, obs, ema):
  maps = 1 if obs == 'bernoulli' else 2
  spec = conv_spec(maps) if net == 'conv' else dense_spec(maps)
  eng, P, cb, x, ki = step_vs_autograd(bk, spec, 6, K, Cs, obs, ema)
  if ema:
    H = eng.hdim
    codes = eng.enc.outs[-1].cpu().numpy().reshape(-1, Cs or H)
    nc, nm, ncb = ema64(codes, ki, np.zeros(K), cb, 0.99, 1e-5)
    close(eng.vq_ema_counts.cpu().numpy(), nc)
    close(eng.vq_ema_means.cpu().numpy(), nm)
    close(eng.vq_codebook.cpu().numpy(), ncb)


@pytest.mark.parametrize('ema', [False, True])
def test_three_train_steps_follow_float64_adam(bk, ema):
  """loss of every step and the parameters after three at the bar of the other models' Adam tests (2e-4 of the
  tensor's largest weight); under the moving average the codebook follows the float64 recursion and Adam's parameter
  vector does not contain it"""
  spec, B, K, Cs, beta, lr = conv_spec(), 4, 5, 8, 1.5, 1e-3
  eng, P, cb, x = vq_case(bk, spec, B, K, Cs, ema=ema, hyper_ring_rows=16)
  ref = VQRef(spec[0], spec[1], 'bernoulli', K, Cs, 0.25, ema, beta)
  P = dict(P)
  if not ema:
    P[('vq', 'codebook')] = cb.copy()
  M = {k: np.zeros_like(v) for k, v in P.items()}
  V = {k: np.zeros_like(v) for k, v in P.items()}
  counts, means, cbk = np.zeros(K), cb.copy(), cb.copy()
  xt = bk.T(x)
  for t in (1, 2, 3):
    nets = {k: v for k, v in P.items() if k[0] != 'vq'}
    cur = cbk if ema else P[('vq', 'codebook')]
    f, G = ref.loss_and_grads(nets, cur, x)
    out = eng.train_step(xt, None, lr=lr, beta=beta).cpu().numpy()
    assert np.array_equal(eng.vq_idx.cpu().numpy(), f['idx']), t   # (no near tie in this case)
    assert abs(out[0] - f['loss']) <= 1e-4 * max(1.0, abs(f['loss'])), (t, out[0], f['loss'])
    if ema:
      counts, means, cbk = ema64(f['codes'], f['idx'], counts, means, 0.99, 1e-5)
    _adam_ref(P, G, M, V, t, lr)
  got = {k: v.cpu().numpy() for k, v in eng.param_views().items()}
  assert set(got) == set(P)
  for k in P:
    assert np.abs(got[k] - P[k]).max() <= 2e-4 * max(1e-3, np.abs(P[k]).max()), k
  if ema:
    assert not any(k[0] == 'vq' for k in got) and eng.params.numel() == eng.m.numel()
    close(eng.vq_codebook.cpu().numpy(), cbk)
    close(eng.vq_ema_means.cpu().numpy(), means)
    close(eng.vq_ema_counts.cpu().numpy(), counts)
  else:
    assert np.abs(got[('vq', 'codebook')] - cb).max() > 1e-4


# ---- 3. engine behaviour ------------------------------------------------------------------------------------------------
def test_plain_engine_call_list_is_unchanged(bk):
  eng, c1 = launch_record(bk, vq_codes=None, vq_code_size=8, vq_commitment=3.0, vq_ema=True)
  assert c1 == PLAIN_STEP_CALLS and eng.vq_K is None
  _, c2 = launch_record(bk, steps=2)
  steady = list(PLAIN_STEP_CALLS)
  steady.remove('odin_slab_reduce_sumsq')
  assert c2 == steady
  nl = len(eng.enc_recs) + len(eng.dec_recs)
  assert eng.range_words.numel() == 2 * nl * RANGE_WORDS
  assert [e[0][0] for e in eng.layout.entries].count('lat') == 2


@pytest.mark.parametrize('ema', [False, True])
def test_vq_codes_adds_the_two_calls_and_drops_the_latent_ones(bk, ema):
  eng, c = launch_record(bk, steps=2, vq_codes=5, vq_code_size=8, vq_ema=ema)
  assert c.count('odin_vq_assign') == 1 and c.count('odin_vq_bwd') == 1
  assert not [n for n in c if 'latent' in n or 'neck' in n or 'rng' in n or 'head' in n or 'tail' in n]
  assert c.index('odin_vq_assign') < c.index('odin_elbo_bernoulli_fwd_bwd_ranged') < c.index('odin_vq_bwd')
  assert c[-1] == 'odin_adam_ring_parts' and c[-2] == 'odin_slab_reduce_sumsq'   # the fused norm survives
  keys = [e[0] for e in eng.layout.entries]
  assert not [k for k in keys if k[0] == 'lat']
  assert (keys[-1] == ('vq', 'codebook')) == (not ema) and ('vq', 'codebook') in keys or ema
  assert eng.dec_recs[0].K == eng.hdim == 24 and eng.vq_L == 3
  if not ema:
    assert set(eng.grad_views()) == set(eng.param_views()) and eng.m.numel() == eng.params.numel()


@pytest.mark.parametrize('ema', [False, True])
def test_range_audit_three_steps(bk, ema):
  eng, P, cb, x = vq_case(bk, conv_spec(), 4, 5, 8, ema=ema)
  audit = RangeAudit(eng)
  seen = []

  def check(e):
    audit(e)
    # the two words of the quantiser: the encoder's top gradient (dcodes) and z_q into the decoder's first layer
    top = e.enc.dy_word[-1]
    assert top == e.enc.word(len(e.enc_recs) - 1)
    if e._vq_zq_word is not None:
      i = (e._vq_zq_word - e.range_words.data_ptr()) // 4
      b = float(e.range_words[i:i + RANGE_WORDS].view(torch.float32).max())
      assert b == float(e.z.abs().max())
      seen.append(b)
  eng.debug_check_ranges = check
  xt = bk.T(x)
  for _ in range(3):
    eng.train_step(xt, None, lr=1e-3, beta=2.0)
    audit.check_cleared()
  assert len(audit.steps) == 3 and audit.n_checked() > 0 and not audit.failures
  audit.check_cover()
  names = [n for n, *_ in audit.steps[0]]
  assert any(n.startswith(f'enc.gouts[{len(eng.enc_recs) - 1}]') for n in names)
  assert (len(seen) == 3) == (eng._vq_zq_word is not None)


@pytest.mark.parametrize('net', ['conv', 'dense'])
def test_run_decoder_on_the_engines_own_z_keeps_its_word(bk, net):
  """encode, then decode the engine's own z_q, twice: the second forward pass resets the activation words (z_q's
  among them) before the decoder reads them, so run_decoder takes the word from its argument whatever tensor it is."""
  eng, P, cb, x = vq_case(bk, conv_spec() if net == 'conv' else dense_spec(), 4, 5, 8)
  eng.run_encoder(bk.T(x))
  ref = eng.run_decoder(eng.z.clone()).clone()
  for _ in range(2):
    eng.run_encoder(bk.T(x))
    out = eng.run_decoder(eng.z)
    assert torch.equal(out, ref)
    if eng._vq_zq_word is not None:
      i = (eng._vq_zq_word - eng.range_words.data_ptr()) // 4
      assert float(eng.range_words[i:i + RANGE_WORDS].view(torch.float32).max()) == float(eng.z.abs().max())


def test_excluded_options_raise_at_construction(bk):
  enc, dec, in_shape, zdim = tiny_spec()
  mk = lambda **kw: VAEEngine(enc, dec, in_shape, zdim, 4, bk.dev, lib=bk.L, **{'vq_codes': 5, **kw})
  for kw, exc, word in ((dict(tc='betatc'), ValueError, 'tc'), (dict(latent_reg='mmd'), ValueError, 'latent_reg'),
                        (dict(vamprior_components=3), ValueError, 'vamprior'),
                        (dict(free_bits=0.5), NotImplementedError, 'free_bits'),
                        (dict(capacity=True), NotImplementedError, 'capacity'),
                        (dict(force_dp=True), NotImplementedError, 'data parallel'),
                        (dict(world_size=2), NotImplementedError, 'data parallel'),
                        (dict(neck_bwd=True), NotImplementedError, 'neck'),
                        (dict(vq_code_size=7), ValueError, 'vq_code_size'),
                        (dict(vq_codes=1025), ValueError, 'vq_codes'),
                        (dict(vq_codes=1024, vq_code_size=24), ValueError, 'quantiser kernel')):
    with pytest.raises(exc, match=word):
      mk(**kw)
  eng = mk()
  assert not (eng.neck or eng.lat_block or eng.fused_tail or eng.gauss_head)
  cb = eng.param_views()[('vq', 'codebook')]
  assert cb.shape == (5, 24) and float(cb.abs().max()) <= math.sqrt(3.0 / 5) and float(cb.abs().max()) > 0.3


# ---- 4. model API ---------------------------------------------------------------------------------------------------
def _vq_model(bk, **kw):
  from odin_ai_amd.vae import VQVAE
  args = dict(n_codes=6, code_size=8, beta=1.5, device=bk.dev, lib=bk.L)
  args.update(kw)
  return VQVAE(**args, **api_nets())


def _api_x(B=6, seed=2):
  return np.clip(np.random.default_rng(seed).random((B, 8, 8, 1)), 1e-6, 1 - 1e-6).astype(np.float32)


def _spread_codebook(vae, seed=11):
  """a codebook among the codes (the default U(+-sqrt(3 / K)) is fine too; this one uses several codes)"""
  eng = vae._engine(1)
  cb = (np.random.default_rng(seed).standard_normal((eng.vq_K, eng.vq_Cs)) * 0.3).astype(np.float32)
  eng.init_codebook(cb)
  return cb.astype(np.float64)


def test_api_names_and_defaults(bk):
  import inspect
  from odin_ai_amd.vae import (BetaVAE, MultinomialPrior, VectorQuantizedPosterior, VectorQuantizer, VQVAE, VQ_LAYER,
                               get_vae)
  assert get_vae('vqvae') is VQVAE and get_vae('vq_vae') is VQVAE
  d = inspect.signature(VQVAE.__init__).parameters
  want = dict(n_codes=64, commitment_weight=0.25, distance_metric='euclidean', trainable_prior=False, ema_decay=0.99,
              ema_update=False, beta=1.0, epsilon=1e-5, code_size=None)
  assert {k: d[k].default for k in want} == want
  vae = VQVAE(device=bk.dev, lib=bk.L, **api_nets())
  assert isinstance(vae, BetaVAE) and isinstance(vae.quantizer, VectorQuantizer) and not vae.ema_update
  q = vae.quantizer
  assert (q.n_codes, q.commitment_weight, q.ema_decay, q.epsilon, q.code_size, q.name) == (64, 0.25, 0.99, 1e-5, 24,
                                                                                            VQ_LAYER)
  assert isinstance(q.prior, MultinomialPrior) and not q.prior.logits.any()
  cb = vae.codebook
  assert cb.shape == (64, 24) and float(cb.abs().max()) <= math.sqrt(3 / 64) and float(cb.std()) > 0.05
  assert vae.ema_counts is None and vae.ema_means is None
  assert vae.variable_name(('vq', 'codebook')) == 'VQLatents/codebook'
  keys = list(vae.trainable_variables)
  assert keys[-1] == ('vq', 'codebook') and not [k for k in keys if k[0] == 'lat']
  ema = _vq_model(bk, ema_update=True)
  assert ema.ema_update and not [k for k in ema.trainable_variables if k[0] == 'vq']
  assert torch.equal(ema.ema_means, ema.codebook) and not ema.ema_counts.any()
  with pytest.raises(ValueError, match='analytic'):
    _vq_model(bk, analytic=False)
  with pytest.raises(NotImplementedError):
    _vq_model(bk, distance_metric='cosine')
  with pytest.raises(NotImplementedError):
    _vq_model(bk, sample_shape=2)
  with pytest.raises(ValueError):
    _vq_model(bk, code_size=7)
  with pytest.raises(NotImplementedError):
    vae.marginal_log_prob(_api_x())
  with pytest.raises(ValueError, match='analytic'):
    vae.set_elbo_configs(analytic=False)
  assert _vq_model(bk, trainable_prior=True).quantizer.trainable_prior   # accepted, without effect


@pytest.mark.parametrize('ema', [False, True])
def test_api_elbo_components_and_optimize(bk, ema):
  vae = _vq_model(bk, ema_update=ema)
  cb = _spread_codebook(vae)
  x = _api_x()
  nets = api_nets()
  ref = VQRef(nets['encoder'].layers, nets['decoder'].layers, 'bernoulli', 6, 8, 0.25, ema, 1.5)
  P = {k: v.detach().cpu().numpy().astype(np.float64) for k, v in vae.trainable_variables.items() if k[0] != 'vq'}
  f, G = ref.loss_and_grads(P, cb, x.astype(np.float64))
  llk, kl = vae.elbo_components(x)
  want = {'kl_latents', 'commitment_latents'} | (set() if ema else {'latents_latents'})
  assert set(llk) == {'llk_image'} and set(kl) == want
  close(llk['llk_image'].cpu().numpy(), f['llk'])
  assert abs(float(kl['kl_latents']) - 1.5 * 3 * math.log(6)) <= 1e-5
  assert abs(float(kl['commitment_latents']) - 0.25 * f['m']) <= 1e-4 * 0.25 * f['m']
  if not ema:
    assert abs(float(kl['latents_latents']) - f['m']) <= 1e-4 * f['m']
  elbo = vae.elbo(llk, kl)
  assert elbo.shape == (6,)
  assert abs(float(elbo.mean()) + f['loss']) <= 1e-4 * max(1.0, abs(f['loss']))
  assert abs(float(elbo.mean()) + float(vae._engine(6).out4[0])) <= 1e-4 * max(1.0, abs(f['loss']))
  loss, metrics = vae.optimize(x, learning_rate=1e-3)
  assert set(metrics) == {'llk_image'} | want
  assert abs(float(loss) - f['loss']) <= 1e-4 * max(1.0, abs(f['loss'])) and vae.step == 1
  assert abs(float(metrics['commitment_latents']) - 0.25 * f['m']) <= 1e-4 * f['m']
  if ema:
    nc, nm, ncb = ema64(f['codes'], f['idx'], np.zeros(6), cb, 0.99, 1e-5)
    close(vae.codebook.cpu().numpy(), ncb)
    close(vae.ema_counts.cpu().numpy(), nc)


def test_api_encode_decode_call_and_sampling(bk):
  from odin_ai_amd.vae import VectorQuantizedPosterior
  vae = _vq_model(bk)
  cb = _spread_codebook(vae)
  x = _api_x(5)
  q = vae.encode(x)
  assert isinstance(q, VectorQuantizedPosterior)
  assert q.codes.shape == (5, 3, 8) and q.assignments.shape == (5, 3) and q.nearest_codes.shape == (5, 3, 8)
  assert q.one_hot().shape == (5, 3, 6) and torch.equal(q.one_hot().argmax(-1).int(), q.assignments)
  assert q.tensor().shape == (5, 24) and torch.equal(q.sample(), q.tensor())
  idx, _, _, _, dist = assign64(q.codes.cpu().numpy().reshape(-1, 8), cb)
  check_assignment(q.assignments.cpu().numpy().reshape(-1), dist)
  assert np.array_equal(q.nearest_codes.cpu().numpy().reshape(-1, 8), cb[q.assignments.cpu().numpy().reshape(-1)])
  assert abs(float(q.commitment_loss) - 0.25 * float(q.latents_loss)) < 1e-7 and float(q.latents_loss) > 0
  assert vae.encode(x, only_encoding=True).shape == (5, 24)
  px = vae.decode(q)
  assert tuple(px.mean().shape) == (5, 8, 8, 1)
  assert vae.decode(q.tensor(), only_decoding=True).shape == (5, 8, 8, 1)
  px2, q2 = vae(x)
  assert torch.equal(px2.mean(), px.mean()) and torch.equal(q2.assignments, q.assignments)
  qz = vae.quantizer
  codes = q.codes.cpu().numpy()
  assert torch.equal(qz.sample_indices(codes).cpu(), q.assignments.cpu())
  assert torch.equal(qz.sample_nearest(codes).cpu(), q.nearest_codes.cpu())
  s = qz.sample(7, seed=3)
  assert s.shape == (7, 8) and torch.equal(s, qz.sample(7, seed=3))
  rows = {tuple(r) for r in cb.astype(np.float32).tolist()}
  assert all(tuple(r) in rows for r in s.cpu().numpy().tolist())
  zp = vae.sample_prior(4, seed=5)
  assert zp.shape == (4, 24) and all(tuple(r) in rows for r in zp.cpu().numpy().reshape(-1, 8).tolist())
  assert tuple(vae.sample_observation(4, seed=5).mean().shape) == (4, 8, 8, 1)
  assert float(qz.prior.log_prob(q.one_hot()).sum(-1).mean()) == pytest.approx(-3 * math.log(6))


@pytest.mark.parametrize('ema', [False, True])
@pytest.mark.parametrize('fmt', ['npz', 'tf'])
def test_api_save_load_round_trip(bk, tmp_path, fmt, ema):
  vae = _vq_model(bk, ema_update=ema)
  _spread_codebook(vae)
  x = _api_x()
  vae.optimize(x, learning_rate=1e-2)
  path = str(tmp_path / 'w')
  vae.save_weights(path, save_format=fmt)
  other = _vq_model(bk, ema_update=ema)
  assert not torch.equal(other.codebook, vae.codebook)
  other.load_weights(path, raise_notfound=True)
  assert other.step == 1 and torch.equal(other.codebook, vae.codebook)
  for k, v in vae.trainable_variables.items():
    assert torch.equal(v, other.trainable_variables[k]), k
  if ema:
    assert torch.equal(other.ema_counts, vae.ema_counts) and torch.equal(other.ema_means, vae.ema_means)
    assert float(vae.ema_counts.sum()) > 0
  a, b = vae.elbo_components(x), other.elbo_components(x)
  assert torch.equal(a[0]['llk_image'], b[0]['llk_image'])
  assert torch.equal(a[1]['commitment_latents'], b[1]['commitment_latents'])


@pytest.mark.parametrize('ema', [False, True])
def test_api_fit_lowers_the_loss_on_two_clusters(bk, ema):
  rng = np.random.default_rng(1)
  protos = (rng.random((2, 8, 8, 1)) < 0.4).astype(np.float32)
  xs = np.clip(protos[rng.integers(0, 2, 32)] * 0.9 + 0.05, 1e-6, 1 - 1e-6).astype(np.float32)
  vae = _vq_model(bk, ema_update=ema, n_codes=4, code_size=None, beta=1.0)
  before, _ = vae.optimize(xs[:16], training=False)
  # (1e-3: Adam's per-step move stays small against the codebook's scale; at 5e-3 the gradient form overshoots after
  # eight steps on this toy set)
  vae.fit(xs, max_iter=12, batch_size=16, learning_rate=1e-3, compile_graph=False)
  after, m = vae.optimize(xs[:16], training=False)
  assert vae.step == 12 and float(after) < float(before), (float(before), float(after))
  assert np.isfinite(float(m['commitment_latents']))
  # engines of two batch sizes read one codebook (under the moving average: the same three tensors)
  e1, e16 = vae._engine(1), vae._engine(16)
  assert e1.vq_codebook.data_ptr() == e16.vq_codebook.data_ptr()
  if ema:
    assert e1.vq_ema_counts.data_ptr() == e16.vq_ema_counts.data_ptr()


# ---- 5. full size on the MI355X ---------------------------------------------------------------------------------------
GPU_NETS = [('dsprites', lambda: vo.dsprites_spec(1)), ('shapes3d', lambda: vo.dsprites_spec(3))]
GPU_VQ = [(64, None), (512, 16), (256, 32)]


@pytest.mark.gpu
@pytest.mark.parametrize('ema', [False, True])
@pytest.mark.parametrize('K,Cs', GPU_VQ)
@pytest.mark.parametrize('name,spec', GPU_NETS, ids=[c[0] for c in GPU_NETS])
def test_gpu_full_size_step(name, spec, K, Cs, ema):
  enc, dec, in_shape, _ = spec()
  eng, *_ = step_vs_autograd(_Hip(), (enc, dec, in_shape), 256, K, Cs, 'bernoulli', ema)
  assert eng.vq_N == 256 * eng.vq_L and not eng.neck


@pytest.mark.gpu
@pytest.mark.parametrize('ema', [False, True])
def test_gpu_graph_replay_equals_eager(ema):
  """five steps: the captured step replays bit for bit what the eager launches compute, the moving-average state
  included"""
  bk = _Hip()
  enc, dec, in_shape, _ = vo.dsprites_spec(1)
  rng = np.random.default_rng(1)
  xs = [bk.T(np.clip(rng.random((256,) + in_shape), 1e-6, 1 - 1e-6)) for _ in range(5)]
  res = []
  for use_graph in (False, True):
    eng, P, cb, _ = vq_case(bk, (enc, dec, in_shape), 256, 512, 16, ema=ema)
    outs, idxs = [], []
    for x in xs:
      outs.append(eng.train_step(x, None, lr=1e-3, beta=1.0, use_graph=use_graph).clone())
      idxs.append(eng.vq_idx.clone())
    torch.cuda.synchronize()
    state = [t.clone() for t in eng.vq_state()] if ema else [eng.vq_codebook.clone()]
    res.append([eng.params.clone(), eng.out8.clone(), torch.stack(outs), torch.stack(idxs)] + state)
  for a, b in zip(res[0], res[1]):
    assert torch.equal(a, b)
  assert bool(torch.isfinite(res[0][2]).all()) and float(res[0][2][:, 3].min()) > 0
  assert not torch.equal(res[0][-1], bk.T(cb))   # the codebook moved
