"""Shared set-up of tests/test_optimizer_step.py: guard-banded buffers, hyper-parameter rows and rings as the engine
lays them out, the float64 oracle of one update, and one harness that runs any of the flat Adam launchers of
pointwise.hip and checks everything a call may and may not write."""
import functools
import math

import numpy as np
import torch

from odin_ai_amd.engine import H_ALPHA, H_BETA, N_HYPER
from oracle import vae_oracle as vo
from tests.test_pointwise import close

F32, F64 = np.float32, np.float64
PAT = 0x5A5AA5A5   # guard words: a bit pattern that reads as a finite float (1.5e16), not NaN
PAD = 64           # guard words on each side: 256 bytes, so an interior pointer keeps torch's 16-byte alignment
WS_FILL = -7.0     # the workspace words no stage-1 workgroup owns

LAUNCHERS = ('step_flat', 'sumsq_adam_flat', 'finalize_flat', 'ring', 'ring+fin', 'ring_parts', 'ring_parts+fin')


def stage1_grid(n):
  """workgroups of the norm's first stage = partials it leaves in the workspace (`n_parts` of odin_adam_ring_parts)"""
  return max(1, min(1024, (n // 4 + 1 + 255) // 256))


class Guard:
  """Buffers inside larger allocations pre-filled with PAT; check(): the surrounding words and every frozen buffer
  are bit-unchanged."""

  def __init__(self, bk):
    self.bk, self.bufs = bk, []

  def buf(self, name, data, dtype=torch.float32, frozen=False):
    src = data if isinstance(data, torch.Tensor) else self.bk.T(np.asarray(data), dtype)
    n = src.numel() * src.element_size() // 4   # (whole 32-bit words)
    assert n * 4 == src.numel() * src.element_size()
    big = torch.full((n + 2 * PAD,), PAT, dtype=torch.int32, device=self.bk.dev)
    view = big[PAD:PAD + n].view(dtype)
    view.copy_(src.reshape(-1))
    assert view.data_ptr() % 16 == 0
    self.bufs.append([name, big, n, None])
    if frozen:
      self.freeze(view)
    return view

  def freeze(self, view=None):
    """snapshot `view` (default: every buffer) as it is now: check() requires it bit-unchanged"""
    for b in self.bufs:
      if view is None or b[1][PAD:].data_ptr() == view.data_ptr():
        b[3] = b[1][PAD:PAD + b[2]].clone()

  def check(self):
    for name, big, n, snap in self.bufs:
      assert bool((big[:PAD] == PAT).all()), f'{name}: written in front of the buffer'
      assert bool((big[PAD + n:] == PAT).all()), f'{name}: written past the buffer'
      if snap is not None:
        assert torch.equal(big[PAD:PAD + n], snap), f'{name}: changed'


# ---------------------------------------------------------------------------------------------- data + oracle ------
@functools.lru_cache(maxsize=2)
def base(n):
  """float32 theta, g, m, v of n elements and the float64 sum of the float32-rounded squared gradients"""
  rng = np.random.default_rng(1000 + n % 9973)
  th, g = rng.standard_normal(n).astype(F32), (rng.standard_normal(n) * 0.3).astype(F32)
  m, v = (rng.standard_normal(n) * 0.1).astype(F32), (rng.random(n) * 0.1).astype(F32)
  for a in (th, g, m, v):
    a.setflags(write=False)
  return th, g, m, v, float((g.astype(F64) ** 2).sum())


def adam_scalars(t, lr, b1=0.9, b2=0.999, eps=1e-7, gs=1.0):
  """the five floats the kernel reads (alpha_t, beta_1, beta_2, epsilon, gradient scale), float32-rounded"""
  b1, b2 = float(F32(b1)), float(F32(b2))
  return np.array([lr * math.sqrt(1 - b2 ** t) / (1 - b1 ** t), b1, b2, eps, gs], F32)


def oracle_update(th, g, m, v, t, lr, sc, clip):
  """float64: tf.clip_by_global_norm on g, the row's gradient scale, Keras Adam with the row's float32 scalars"""
  with np.errstate(all='ignore'):
    g64 = np.asarray(g, F64)
    if clip > 0.0:
      g64 = vo.clip_by_global_norm([g64], float(F32(clip)))[0][0]
    return vo.adam_keras(np.asarray(th, F64), g64 * float(sc[4]), np.asarray(m, F64), np.asarray(v, F64), t, lr,
                         b1=float(sc[1]), b2=float(sc[2]), eps=float(sc[3]))


def clip_for(mode, g2):
  """'off' | 'active' (half the norm) | 'inactive' (1.5 x the norm: the branch cannot flip on rounding)"""
  return {'off': 0.0, 'active': float(F32(0.5 * math.sqrt(g2))), 'inactive': float(F32(1.5 * math.sqrt(g2)))}[mode]


@functools.lru_cache(maxsize=2)
def matrix_oracle(n, mode):
  th, g, m, v, g2 = base(n)
  _, sc, lr, _, _ = Rows(LAYOUTS[N_HYPER + 4])(T0)
  return oracle_update(th, g, m, v, T0, lr, sc, clip_for(mode, g2))


T0 = 6   # (an even step: the row behind it carries a learning rate 100 x as large)


@functools.lru_cache(maxsize=None)
def fin_data(B, n_part):
  rng = np.random.default_rng(21 + B)
  return (rng.standard_normal((B, n_part)) * 30).astype(F32), (rng.random(B) * 5).astype(F32), F32(0.37)


def fin_oracle(part, kl, beta, tcw, tcv):
  """the float64 reference of tests/test_pointwise.py::test_elbo_finalize_partial_counts, with the TC term"""
  ref = part.astype(F64).sum(1)
  ml, mk = ref.mean(), float(beta) * kl.astype(F64).mean()
  tc = float(tcw) * float(tcv) if tcv is not None else 0.0
  return ref, [-(ml - mk - tc), ml, mk, tc]


# ---------------------------------------------------------------------------------------------- rows and rings ------
class Layout:
  """where a hyper-parameter row keeps the step number, Adam's five scalars and the ELBO weights (beta, TC weight).
  alpha_off None: the row is too short for the five scalars -- they live in a buffer of their own (the staged row of
  odin_adam_ring_parts is then longer than the ring's rows and holds them at word 8)."""

  def __init__(self, rf, t_word, alpha_off, elbo_off):
    self.rf, self.t_word, self.alpha_off, self.elbo_off = rf, t_word, alpha_off, elbo_off
    self.staged_alpha = 8 if alpha_off is None else alpha_off
    self.staged_len = max(rf, self.staged_alpha + 5, 8)


LAYOUTS = {5: Layout(5, 3, None, 0), N_HYPER + 4: Layout(N_HYPER + 4, N_HYPER, H_ALPHA, H_BETA),
           24: Layout(24, 21, 4, 12), 64: Layout(64, 63, 40, 7)}


class Rows:
  """step t -> (row of floats, Adam scalars, lr, beta, tcw): every word distinct and random, the learning rate of
  odd steps 100 x and their beta 10 x the even steps', so a kernel that read its neighbour's row misses by far"""

  def __init__(self, lay, seed=0):
    self.lay, self.seed, self.tab = lay, seed, {}

  def __call__(self, t):
    if t not in self.tab:
      lay, rng = self.lay, np.random.default_rng(7919 * self.seed + t)
      row = (1.0 + rng.random(lay.rf) + t).astype(F32)
      lr = 1e-3 * (100.0 if t & 1 else 1.0) * (1 + 0.1 * rng.random())
      sc = adam_scalars(t, lr, 0.85 + 0.1 * rng.random(), 0.99 + 0.009 * rng.random(), 1e-7, 0.5 + rng.random())
      beta, tcw = F32((10.0 if t & 1 else 1.0) * (1 + rng.random())), F32(1 + rng.random())
      if lay.alpha_off is not None:
        row[lay.alpha_off:lay.alpha_off + 5] = sc
      row[lay.elbo_off:lay.elbo_off + 2] = (beta, tcw)
      row.view(np.int32)[lay.t_word] = t
      self.tab[t] = (row, sc, lr, beta, tcw)
    return self.tab[t]

  def ring(self, rows, t0):
    """the ring as the engine has filled it when step t0 runs: slot s holds the next step after t0 that maps to it"""
    out = np.zeros((rows, self.lay.rf), F32)
    for t in range(t0 + 1, t0 + rows + 1):
      out[t % rows] = self(t)[0]
    return out


def ptr(t, off=0):
  return None if t is None else t.data_ptr() + 4 * off


class Harness:
  """theta, m, v, g and every buffer a launcher touches, guard-banded; step() runs one launcher for the step whose row
  `cur` holds and checks all of it: results against the float64 oracle and bit for bit against odin_adam_step_flat,
  the norm, the ELBO outputs, the ring advance and the bytes that must not change."""

  def __init__(self, bk, th, g, m, v, *, lay=None, rows=8, t0=T0, table=None, flag=True, fin=None, tc=False,
               no_ring=False):
    self.bk, self.L, self.n = bk, bk.L, len(th)
    self.lay = lay = lay or LAYOUTS[N_HYPER + 4]
    self.rows, self.t, self.table = rows, t0, table or Rows(lay)
    self.no_ring = no_ring
    G = self.G = Guard(bk)
    self.th, self.m, self.v = G.buf('theta', th), G.buf('m', m), G.buf('v', v)
    self.g = G.buf('g', g, frozen=True)
    self.ws = G.buf('workspace', np.full(1024, WS_FILL))
    self.gn = G.buf('gnorm2_out', np.zeros(1))
    self.flag = G.buf('flag', np.zeros(1), torch.int32) if flag else None
    self.cur = G.buf('cur', self.table(t0)[0])
    self.ring = G.buf('ring', self.table.ring(rows, t0), frozen=True)
    self.hyper = G.buf('hyper', np.zeros(5))          # Adam's scalars where the row does not hold them
    self.staged = G.buf('staged', np.full(lay.staged_len, -3.0))
    self.fin, self.tc = fin, None
    if fin is not None:
      part, kl, tcv = fin_data(*fin)
      self.part, self.kl = G.buf('llk_part', part, frozen=True), G.buf('kl', kl, frozen=True)
      self.tc = G.buf('tc', [tcv], frozen=True) if tc else None
      self.llk, self.out4 = G.buf('llk', np.zeros(fin[0])), G.buf('out4', np.zeros(4))
    self.h64 = None   # (the free-running float64 state of a sequence of steps)

  # -- one call ------------------------------------------------------------------------------------------------------
  def launch(self, launcher, clip, raw=False, **over):
    """-> the launcher's return code.  raw: through ctypes, no exception on an error; over: arguments replaced"""
    L, lay, n = (self.L.c if raw else self.L), self.lay, self.n
    row, sc, lr, beta, tcw = self.table(self.t)
    a = (ptr(self.th), ptr(self.g), ptr(self.m), ptr(self.v), n)
    fl = ptr(self.flag)
    fin = self.fin is not None and (launcher.endswith('+fin') or launcher == 'finalize_flat')
    B, n_part = self.fin if fin else (0, 0)
    part, kl, tc, llk, out4 = (ptr(self.part), ptr(self.kl), ptr(self.tc), ptr(self.llk), ptr(self.out4)) if fin else (None,) * 5
    in_row = lay.alpha_off is not None
    self.hyper.copy_(self.bk.T(sc))
    name = launcher.split('+')[0]
    if name in ('step_flat', 'sumsq_adam_flat', 'finalize_flat'):
      hy, eh = ptr(self.hyper), ptr(self.cur, lay.elbo_off)
      if name == 'step_flat':
        self.L.odin_sumsq_flat(ptr(self.g), n, ptr(self.ws), ptr(self.gn), None)
        return self._call(raw, L.odin_adam_step_flat, *a, hy, ptr(self.gn), clip, fl, None)
      if name == 'sumsq_adam_flat':
        return self._call(raw, L.odin_sumsq_adam_flat, *a, hy, ptr(self.ws), ptr(self.gn), clip, fl, None)
      return self._call(raw, L.odin_sumsq_adam_finalize_flat, *a, hy, ptr(self.ws), ptr(self.gn), clip, fl, part, n_part,
                        kl, eh, tc, llk, out4, B, None)
    rg = dict(ring=ptr(self.ring), cur=ptr(self.cur), staged=ptr(self.staged), rows=self.rows, row_floats=lay.rf,
              t_word=lay.t_word, n_parts=stage1_grid(n))
    rg.update(over)
    if name == 'ring':
      # as engine.adam: Adam's scalars and the ELBO weights are read from `cur`, which this very call advances
      hy = ptr(self.cur, lay.alpha_off) if in_row else ptr(self.hyper)
      return self._call(raw, L.odin_sumsq_adam_ring, *a, hy, ptr(self.ws), ptr(self.gn), clip, fl, part, n_part, kl,
                        ptr(self.cur, lay.elbo_off), tc, llk, out4, B, rg['ring'], rg['cur'], rg['staged'], rg['rows'],
                        rg['row_floats'], rg['t_word'], None)
    assert name == 'ring_parts'
    # the producer's part (odin_slab_reduce_sumsq in the engine): the stage-1 partials in the workspace -- here those
    # odin_sumsq_adam_flat leaves, run on copies that are the bit-exact reference of this call -- and the staged row
    if not over.get('keep_parts'):
      self.twin = [self.th.clone(), self.m.clone(), self.v.clone(), self.bk.zeros(1),
                   self.bk.zeros(1, dtype=torch.int32)]
      tw = self.twin
      self.L.odin_sumsq_adam_flat(ptr(tw[0]), ptr(self.g), ptr(tw[1]), ptr(tw[2]), n, ptr(self.hyper), ptr(self.ws),
                                  ptr(tw[3]), clip, ptr(tw[4]) if self.flag is not None else None, None)
    st = np.full(lay.staged_len, -3.0, F32)
    st[:lay.rf] = row
    st[lay.staged_alpha:lay.staged_alpha + 5] = sc
    self.staged.copy_(self.bk.T(st))
    self.G.freeze(self.staged)
    self.G.freeze(self.ws)
    if self.no_ring:
      rg['ring'] = None
      self.G.freeze(self.cur)
    return self._call(raw, L.odin_adam_ring_parts, *a, rg['staged'], lay.staged_alpha, lay.elbo_off,
                      over.get('parts', ptr(self.ws)), rg['n_parts'], ptr(self.gn), clip, fl, part, n_part, kl, tc, llk,
                      out4, B, rg['ring'], rg['cur'], rg['rows'], rg['row_floats'], rg['t_word'], None)

  def _call(self, raw, fn, *args):
    if raw:   # a call that is expected to be refused: every buffer as it is now must survive it
      self.G.freeze()
    return fn(*args)

  def step(self, launcher, clip, g2_ref, ref=None, skipped=False, finite=None):
    """run `launcher` for step self.t and check it.  ref: the oracle's (theta, m, v) -- default: one float64 update of
    the state before the call; skipped: a non-finite gradient with a flag -- nothing is updated; finite: the mask of
    elements to compare (non-finite gradient without a flag)"""
    bk, lay, n, t = self.bk, self.lay, self.n, self.t
    name = launcher.split('+')[0]
    row, sc, lr, beta, tcw = self.table(t)
    before = [x.clone() for x in (self.th, self.m, self.v)]
    if ref is None and not skipped:
      ref = oracle_update(*(x.cpu().numpy() for x in before[:1]), self.g.cpu().numpy(),
                          *(x.cpu().numpy() for x in before[1:]), t, lr, sc, clip)
    self.launch(launcher, clip)
    self.G.check()
    # the norm: float64 sum of the float32-rounded squares, any order of <= ~40 chained non-negative additions
    gn = float(self.gn.item())
    if math.isfinite(g2_ref):
      assert abs(gn - g2_ref) <= 1e-5 * g2_ref, (gn, g2_ref)
    else:
      assert not math.isfinite(gn)
    assert bool((self.ws[stage1_grid(n):] == WS_FILL).all()), 'workspace written past the stage-1 grid'
    if name in ('finalize_flat', 'ring'):   # the same stage-1 partition as odin_sumsq_flat
      ws2, out2 = bk.zeros(1024), bk.zeros(1)
      self.L.odin_sumsq_flat(ptr(self.g), n, ptr(ws2), ptr(out2), None)
      assert torch.equal(out2.view(torch.int32), self.gn.view(torch.int32))
      assert torch.equal(ws2[:stage1_grid(n)].view(torch.int32), self.ws[:stage1_grid(n)].view(torch.int32))
    got = (self.th, self.m, self.v)
    if skipped:
      assert int(self.flag.item()) == 1
      for x, y in zip(got, before):
        assert torch.equal(x.view(torch.int32), y.view(torch.int32))
    else:
      if self.flag is not None:
        assert int(self.flag.item()) == 0
      for x, y in zip(got, ref):
        x = x.cpu().numpy()
        if finite is not None:
          assert not np.isfinite(x[~finite]).any()
          x, y = x[finite], y[finite]
        close(x, y, 1e-6)
      # bit identity across launchers: odin_adam_step_flat on copies, fed this call's norm and this step's scalars
      c, old = before, bk.T(sc)
      self.L.odin_adam_step_flat(ptr(c[0]), ptr(self.g), ptr(c[1]), ptr(c[2]), n, ptr(old), ptr(self.gn), clip, None,
                                 None)
      for x, y in zip(got, c):
        assert torch.equal(x.view(torch.int32), y.view(torch.int32))
    if name == 'ring_parts':   # ... and odin_sumsq_adam_flat, whose partials it summed
      tw = self.twin
      for x, y in zip(got + (self.gn,), tw[:4]):
        assert torch.equal(x.view(torch.int32), y.view(torch.int32))
    # the ring: advanced by every call, a skipped step included (engine.py counts every step)
    if name in ('ring', 'ring_parts') and not self.no_ring:
      nxt = bk.T(self.table(t + 1)[0])
      assert torch.equal(self.cur.view(torch.int32), nxt.view(torch.int32))
      assert torch.equal(self.cur.view(torch.int32), self.ring.view(-1, lay.rf)[(t + 1) % self.rows].view(torch.int32))
      assert int(self.cur.view(torch.int32)[lay.t_word].item()) == t + 1
    if name == 'ring':
      assert torch.equal(self.staged[:5].view(torch.int32), bk.T(sc).view(torch.int32))
      assert bool((self.staged[5:] == -3.0).all())
    # the ELBO outputs: this step's beta / TC weight, bit-equal to the stand-alone launch
    if self.fin is not None and (launcher.endswith('+fin') or name == 'finalize_flat'):
      B, n_part = self.fin
      part, kl, tcv = fin_data(B, n_part)
      llk2, out2, eh = bk.zeros(B), bk.zeros(4), bk.T([beta, tcw])
      self.L.odin_elbo_finalize(ptr(self.part), n_part, ptr(self.kl), ptr(eh), ptr(self.tc), ptr(llk2), ptr(out2), B,
                                None)
      assert torch.equal(self.llk.view(torch.int32), llk2.view(torch.int32))
      assert torch.equal(self.out4.view(torch.int32), out2.view(torch.int32))
      rl, ro = fin_oracle(part, kl, beta, tcw, tcv if self.tc is not None else None)
      close(self.llk.cpu().numpy(), rl, 1e-5)
      close(self.out4.cpu().numpy(), ro, 1e-5)
    # the host's part of the ring: the slot just consumed gets the row of step t + 1 + rows
    if name in ('ring', 'ring_parts') and not self.no_ring:
      self.ring.view(-1, lay.rf)[(t + 1) % self.rows].copy_(bk.T(self.table(t + 1 + self.rows)[0]))
      self.G.freeze(self.ring)
    else:
      self.cur.copy_(bk.T(self.table(t + 1)[0]))   # (a caller that writes the row itself every step)
    self.t = t + 1
