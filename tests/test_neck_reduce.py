"""odin_neck_bwd_reduce + odin_slab_reduce_sumsq_masked (neck.hip / wgrad.hip / slab_reduce.h): a part of the step's slab
reduction executed by extra workgroups of the neck's backward launch, the rest by the step's last reduction -- ONE plan,
two launches.  Every comparison here is bit for bit (int32 views): the same code sums the same rows in the same order and
every norm partial lands at its old index, so there is no tolerance anywhere.

Op level: the neck regime at its smallest (input [B, 8, 8, 64], P = 128, D = 10, C0 = 8; B = 2, 3, 8: 1, 2, 4 neck
workgroups, B = 3 with a ragged last pair), synthetic slabs for the early jobs, every buffer between guard bands.  The
reference is odin_neck_bwd followed by the unmasked odin_slab_reduce_sumsq on an identical world.  Engine level: a
dSprites engine (B = 4, 256) with the option on and off, eager and as a graph, and the call record."""
import ctypes as C

import numpy as np
import pytest
import torch

from odin_ai_amd import _lib
from odin_ai_amd._lib import OdinError, ReduceJob

P_, D_, C0_ = 128, 10, 8
GUARD = 64                      # floats of sentinel on both sides of every buffer (a multiple of 4: alignment is kept)
SENT = 0x5A5A5A5A               # as a float: 1.5e16 -- any sum that touched it shows


# early job sets: (n, rows, stride or 0)
LONG = ([(4096, r, 0) for r in (0, 1, 5, 33, 256)] +          # wide path: 16 virtual blocks each
        [(4100, 7, 4128)] +                                   # wide, ragged: 1025 float4 columns, 17 blocks, padded rows
        [(64, r, 0) for r in (1, 17, 128)] +                  # narrow vector path: one block each
        [(33, 256, 65), (1, 3, 0)] +                          # odd path: 2 blocks / 1 block
        [(4133, 5, 0)])                                       # odd and wider than the grid (gx = 128 from the neck's
#                                                               8192-float slab): 130 blocks, blocks 0 and 1 take two
#                                                               column steps -- every other virtual block runs a guarded one
SHORT = [(64, 17, 0)]                                         # one virtual block: fewer than any reducer count x 4


def _guarded(dev, n, fill=None):
  """-> (whole buffer with guard bands, the n floats between them); `fill`: float values, else the sentinel"""
  buf = torch.full((n + 2 * GUARD,), SENT, dtype=torch.int32, device=dev).view(torch.float32)
  mid = buf[GUARD:GUARD + n]
  if fill is not None:
    mid.copy_(torch.as_tensor(np.ascontiguousarray(fill), dtype=torch.float32))
  return buf, mid


class World:
  """every buffer of one op-level case, the same bits at every construction with the same arguments"""

  def __init__(self, L, dev, B, early):
    self.L, self.dev, self.B, self.early = L, dev, B, early
    rng = np.random.default_rng(100 * B + len(early))
    f = lambda *s: (rng.standard_normal(s) * 0.3).astype(np.float32)
    N0, J = 16 * C0_, 2 * D_
    T = lambda a: torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float32).to(dev)
    xin = torch.nn.functional.elu(torch.tensor(f(B, 8, 8, 64))).numpy()
    src = dict(x=xin, w3=f(4, 4, 64, 64) * 0.1, b3=f(64), w4=f(1024, P_) * 0.1, b4=f(P_), wl=f(P_, J) * 0.3, bl=f(J),
               eps=f(B, D_), w0=f(D_, N0), b0=f(N0), w1=f(4, 4, 64, C0_), b1=f(64), dy1=f(B, 8, 8, 64))
    self.T = {k: T(v) for k, v in src.items()}
    fwd = dict(y3=(B, 4, 4, 64), y4=(B, P_), p=(B, J), z=(B, D_), kl=(B,), fbmask=(B,), y0=(B, N0), y1=(B, 8, 8, 64))
    self.F = {k: torch.zeros(s, dtype=torch.float32, device=dev) for k, s in fwd.items()}
    rows = L.odin_neck_rows(B, P_, D_, C0_)
    assert rows == (B + 1) // 2
    self.rows = rows
    # the neck's outputs between guard bands
    bwd = dict(dz=B * D_, dp=B * J, dh4=B * P_, dy3=B * 1024, dx=B * 4096, slab1=rows * 16 * 64 * C0_,
               slab0=rows * (D_ * N0 + N0), slabl=rows * (P_ * J + J))
    self.O = {k: _guarded(dev, n) for k, n in bwd.items()}
    self.klw = T([0.7])
    self.step = torch.zeros(1, dtype=torch.int32, device=dev)
    self.words = torch.zeros(5 * 2048, dtype=torch.int32, device=dev)
    wp = lambda i: self.words.data_ptr() + 4 * 2048 * i
    L.odin_absmax(self.T['x'].data_ptr(), self.T['x'].numel(), wp(0), None)
    A = _lib.NeckArgs()
    A.B, A.P, A.D, A.C0 = B, P_, D_, C0_
    A.act2, A.act3, A.act4, A.act0, A.act1 = 1, 1, 0, 0, 1
    A.analytic, A.free_bits, A.seed = 0, -1.0, 1
    A.step_dev = self.step.data_ptr()
    for k in ('x', 'w3', 'b3', 'w4', 'b4', 'wl', 'bl', 'w0', 'b0', 'w1', 'b1', 'dy1'):
      setattr(A, k, self.T[k].data_ptr())
    A.eps_in = A.eps = self.T['eps'].data_ptr()
    for k in self.F:
      setattr(A, k, self.F[k].data_ptr())
    for k in bwd:
      setattr(A, k, self.O[k][1].data_ptr())
    A.klw = self.klw.data_ptr()
    A.x_amax, A.y1_amax, A.dh4_amax, A.dy3_amax, A.dx_amax = wp(0), wp(1), wp(2), wp(3), wp(4)
    self.A = A
    L.odin_neck_fwd(C.byref(A), None)
    # ---- the job list: the early jobs on synthetic slabs, the neck's three slabs, the range-word reset
    late = [(16 * 64 * C0_, rows, 0, self.O['slab1'][1]), (D_ * N0 + N0, rows, 0, self.O['slab0'][1]),
            (P_ * J + J, rows, 0, self.O['slabl'][1])]
    offs, o = [], 0
    for n, _, _ in list(early) + [t[:3] for t in late]:
      offs.append(o)
      o += (n + 3) & ~3
    self.g_buf, self.g = _guarded(dev, o)
    self.slabs = []
    jobs = []
    for i, (n, r, st) in enumerate(early):
      w = st if st else n
      sb, s = _guarded(dev, max(1, r) * w, fill=f(max(1, r) * w))
      self.slabs.append((sb, sb.clone()))
      jobs.append(ReduceJob(s.data_ptr(), self.g[offs[i]:].data_ptr(), n, r, st, 0))
    for i, (n, r, st, s) in enumerate(late):
      jobs.append(ReduceJob(s.data_ptr(), self.g[offs[len(early) + i]:].data_ptr(), n, r, st, 0))
    self.rw_buf, self.rw = _guarded(dev, 96, fill=f(96))
    jobs.append(ReduceJob(self.rw.data_ptr(), self.rw.data_ptr(), 96, 0, 96, 0))
    self.offs = offs
    self.n_jobs = len(jobs)
    self.jobs = (ReduceJob * len(jobs))(*jobs)
    self.mask = (1 << len(early)) - 1
    self.part_buf, self.part = _guarded(dev, 2048)
    self.hyper = T(f(24))
    self.staged_buf, self.staged = _guarded(dev, 24)
    self.nparts = C.c_int(0)

  def sync(self):
    if self.dev != 'cpu':
      torch.cuda.synchronize()

  def reduce_args(self):
    return (self.g.data_ptr(), self.g.numel(), self.part.data_ptr(), C.byref(self.nparts), self.hyper.data_ptr(),
            self.staged.data_ptr(), 24, None)

  def run_reference(self):
    L = self.L
    L.odin_neck_bwd(C.byref(self.A), None)
    L.odin_slab_reduce_sumsq(self.jobs, self.n_jobs, *self.reduce_args())
    self.sync()

  def run_split(self, nred, check_between=True):
    L = self.L
    L.odin_neck_bwd_reduce(C.byref(self.A), self.jobs, self.n_jobs, self.mask, self.g.data_ptr(), self.g.numel(),
                           self.part.data_ptr(), nred, None)
    assert L.odin_debug_last_path().decode() == 'neck_bwd_reduce'
    self.sync()
    mid = self.g.clone()
    L.odin_slab_reduce_sumsq_masked(self.jobs, self.n_jobs, self.mask, *self.reduce_args())
    self.sync()
    if check_between:
      ne = len(self.early)
      gi, mi = self.g.view(torch.int32), mid.view(torch.int32)
      for i, (n, _, _) in enumerate(self.early):
        # the masked reduction leaves an early job's range exactly as the neck launch wrote it ...
        assert torch.equal(gi[self.offs[i]:self.offs[i] + n], mi[self.offs[i]:self.offs[i] + n]), ('early range', i)
        assert not bool((mi[self.offs[i]:self.offs[i] + n] == SENT).any()), ('early job not executed by the neck launch', i)
      # ... and the neck launch wrote nothing of the late jobs
      assert bool((mi[self.offs[ne]:] == SENT).all()), 'the neck launch wrote into a late job\'s range'

  def state(self):
    """everything a run may have written, guard bands included, as int32"""
    out = dict(g=self.g_buf, part=self.part_buf, staged=self.staged_buf, rw=self.rw_buf, words=self.words.view(torch.float32))
    out.update({k: v[0] for k, v in self.O.items()})
    out.update({f'slab{i}': sb for i, (sb, _) in enumerate(self.slabs)})
    return {k: v.view(torch.int32).cpu().clone() for k, v in out.items()}, self.nparts.value

  def check_guards(self):
    for name, buf in [('g', self.g_buf), ('part', self.part_buf), ('staged', self.staged_buf), ('rw', self.rw_buf)] + \
                     [(k, v[0]) for k, v in self.O.items()]:
      b = buf.view(torch.int32)
      assert bool((b[:GUARD] == SENT).all()) and bool((b[-GUARD:] == SENT).all()), ('guard band', name)
    for i, (sb, sb0) in enumerate(self.slabs):
      assert torch.equal(sb.view(torch.int32), sb0.view(torch.int32)), ('an input slab was written', i)
    # beyond the partials of the plan nothing is written
    assert bool((self.part.view(torch.int32)[self.nparts.value:] == SENT).all())


def _identity_case(L, dev, B, early, nred):
  ref = World(L, dev, B, early)
  ref.run_reference()
  want, n_want = ref.state()
  ref.check_guards()
  assert 0 < n_want <= 2048
  got2 = None
  for _ in range(2):   # (two runs of the new path: the same bits as each other, too)
    w = World(L, dev, B, early)
    w.run_split(nred)
    got, n_got = w.state()
    w.check_guards()
    assert n_got == n_want
    for k in want:
      assert torch.equal(got[k], want[k]), (k, int((got[k] != want[k]).sum()))
    if got2 is not None:
      for k in got:
        assert torch.equal(got[k], got2[k]), ('second run', k)
    got2 = got
  # the reference did something: every early range and the neck's outputs were written
  assert not bool((want['g'][GUARD:-GUARD] == SENT).all()) and not bool((want['dx'][GUARD:-GUARD] == SENT).any())


def test_identity_on_the_simulator():
  """B = 2 on the CPU build of the same sources: the long job list on one reducer workgroup and on the default count"""
  from tests.simutil import sim_lib
  L = sim_lib()
  _identity_case(L, 'cpu', 2, LONG, 1)
  _identity_case(L, 'cpu', 2, SHORT, -1)


@pytest.mark.gpu
@pytest.mark.parametrize('B', [2, 3, 8])
@pytest.mark.parametrize('early,nred', [(LONG, 1), (LONG, 3), (LONG, -1), (SHORT, 3), (SHORT, -1)],
                         ids=['long-1', 'long-3', 'long-default', 'short-3', 'short-default'])
def test_identity_on_the_gpu(B, early, nred):
  _identity_case(_lib.load(), 'cuda:0', B, early, nred)


def _rejections(L, dev):
  w = World(L, dev, 2, LONG)
  before, _ = w.state()
  # the dry run reports the count of the whole list, with and without the mask
  n0, n1, n2 = C.c_int(-1), C.c_int(-1), C.c_int(-1)
  L.odin_slab_reduce_sumsq(w.jobs, w.n_jobs, w.g.data_ptr(), w.g.numel(), None, C.byref(n0), None, None, 0, None)
  L.odin_slab_reduce_sumsq_masked(w.jobs, w.n_jobs, w.mask, w.g.data_ptr(), w.g.numel(), None, C.byref(n1), None, None, 0,
                                  None)
  L.odin_slab_reduce_sumsq_masked(w.jobs, w.n_jobs, 0, w.g.data_ptr(), w.g.numel(), None, C.byref(n2), None, None, 0, None)
  assert n0.value == n1.value == n2.value > 0
  L.odin_neck_bwd_reduce(C.byref(w.A), w.jobs, w.n_jobs, w.mask, w.g.data_ptr(), w.g.numel(), None, 1, None)   # dry run
  args = lambda jobs, n, mask: (C.byref(w.A), jobs, n, mask, w.g.data_ptr(), w.g.numel(), w.part.data_ptr(), 1, None)
  many = (ReduceJob * 65)(*([w.jobs[0]] * 65))
  outside = (ReduceJob * w.n_jobs)(*w.jobs)
  outside[1].dst = w.rw.data_ptr()   # an early job that writes outside [g, g + g_n)
  for a in (args(many, 65, 1), args(outside, w.n_jobs, w.mask), args(w.jobs, w.n_jobs, w.mask | (1 << (w.n_jobs - 1)))):
    with pytest.raises(OdinError, match=r'rc=-2'):
      L.odin_neck_bwd_reduce(*a)
  for jobs, n, mask in ((many, 65, 1), (outside, w.n_jobs, w.mask), (w.jobs, w.n_jobs, w.mask | (1 << (w.n_jobs - 1)))):
    with pytest.raises(OdinError, match=r'rc=-2'):
      L.odin_slab_reduce_sumsq_masked(jobs, n, mask, *w.reduce_args())
  w.sync()
  after, _ = w.state()
  for k in before:   # nothing was launched: not a bit of any buffer changed
    assert torch.equal(before[k], after[k]), k


def test_rejections_on_the_simulator():
  from tests.simutil import sim_lib
  _rejections(sim_lib(), 'cpu')


@pytest.mark.gpu
def test_rejections_on_the_gpu():
  _rejections(_lib.load(), 'cuda:0')


# ---- engine level ------------------------------------------------------------------------------------------------------
def _dsprites_engine(B, dev, lib=None, **kw):
  from odin_ai_amd.engine import VAEEngine
  from oracle import vae_oracle as vo
  from tests.parity_util import make_case
  spec = vo.dsprites_spec(1)
  enc, dec, in_shape, zdim, x, eps = make_case(spec, 'bernoulli', B)
  kw = dict(kw)
  if lib is not None:
    kw['lib'] = lib
  eng = VAEEngine(enc, dec, in_shape, zdim, B, dev, **kw)
  g = torch.Generator().manual_seed(7)
  eng.params.copy_((torch.randn(eng.params.numel(), generator=g) * 0.05).to(eng.params.device))
  return eng, torch.as_tensor(x, dtype=torch.float32).to(dev), torch.as_tensor(eps, dtype=torch.float32).to(dev)


def _three_steps(B, dev, neck_reduce, use_graph, lib=None):
  eng, x, eps = _dsprites_engine(B, dev, lib=lib, neck_reduce=neck_reduce)
  out = []
  for _ in range(3):
    o4 = eng.train_step(x, eps, lr=1e-3, beta=4.0, use_graph=use_graph)
    if dev != 'cpu':
      torch.cuda.synchronize()
    out.append([t.detach().view(torch.int32).cpu().clone() for t in (o4, eng.llk, eng.kl, eng.grads, eng.params, eng.m, eng.v)])
  return eng, out


@pytest.mark.gpu
@pytest.mark.parametrize('B', [4, 256])
def test_engine_steps_are_bit_identical(B):
  """three steps from the same seed, option on / off x eager / graph: loss terms, gradients, parameters, Adam moments"""
  runs = {}
  for on in (False, True):
    for graph in (False, True):
      eng, runs[on, graph] = _three_steps(B, 'cuda:0', on, graph)
      assert eng._bwd_neck()
      assert any(eng._nr_plans.values()) == on, 'the option did not take (or took where it is off)'
  want = runs[False, False]
  for key, got in runs.items():
    for s in range(3):
      for i, (a, b) in enumerate(zip(got[s], want[s])):
        assert torch.equal(a, b), (key, 'step', s, 'tensor', i, int((a != b).sum()))
  assert float(want[2][3].view(torch.float32).abs().max()) > 0


def _names(calls):
  return [c if isinstance(c, str) else c[0] for c in calls]


def _neck128_engine(dev, lib, **kw):
  """the small engine of the call-record tests whose neck runs its backward launch (quick on the simulator)"""
  from odin_ai_amd.engine import VAEEngine
  from tests.engine_util import case_data, neck_spec
  spec = neck_spec(4, 128)
  x, eps = case_data(dev, spec)
  return VAEEngine(*spec, 4, dev, lib=lib, **kw), x, eps


def _engine_calls(L, dev, make):
  """the on-path issues odin_neck_bwd_reduce in place of odin_neck_bwd and the masked reduction in place of the plain
  one, and no other difference -- from the second step on: the first records the job list and is the off-path"""
  from tests.engine_util import Recorder
  rec = {}
  for on in (False, True):
    calls = []
    eng, x, eps = make(dev, lib=Recorder(L, calls), neck_reduce=on)
    steps = []
    for _ in range(3):
      calls.clear()
      eng.train_step(x, eps, lr=1e-3, beta=4.0)
      steps.append(list(calls))
    rec[on] = steps
    assert eng._bwd_neck()
  assert rec[True][0] == rec[False][0]
  swap = {'odin_neck_bwd': 'odin_neck_bwd_reduce', 'odin_slab_reduce_sumsq': 'odin_slab_reduce_sumsq_masked'}
  # (the second step also asks once whether the neck leaves the reducers enough CUs: a query, no launch)
  assert [st.count('odin_neck_reduce_workgroups') for st in rec[True]] == [0, 1, 0]
  for s in (1, 2):
    off, on = rec[False][s], [c for c in rec[True][s] if c != 'odin_neck_reduce_workgroups']
    assert off.count('odin_neck_bwd') == 1 and off.count('odin_slab_reduce_sumsq') == 1
    assert on == [swap.get(c, c) for c in off]


def test_engine_calls_on_the_simulator():
  from tests.simutil import sim_lib
  _engine_calls(sim_lib(), 'cpu', _neck128_engine)


@pytest.mark.gpu
def test_engine_calls_on_the_gpu():
  _engine_calls(_lib.load(), 'cuda:0', lambda dev, **kw: _dsprites_engine(4, dev, **kw))


def _shapes3d_calls(L, dev):
  """P = 256: the neck's backward launch is off, and the option changes no call"""
  from odin_ai_amd.engine import VAEEngine
  from tests.engine_util import Recorder, case_data, neck_spec
  spec = neck_spec(5, 256)
  x, eps = case_data(dev, spec)
  rec = []
  for on in (False, True):
    calls = []
    eng = VAEEngine(*spec, 4, dev, lib=Recorder(L, calls, args=True), neck_reduce=on)
    for _ in range(2):
      eng.train_step(x, eps, lr=1e-3, beta=2.0)
    assert eng.neck and not eng._bwd_neck()
    rec.append(calls)
  assert rec[0] == rec[1] and 'odin_neck_bwd_reduce' not in _names(rec[1])


def test_shapes3d_neck_issues_the_same_calls_on_the_simulator():
  from tests.simutil import sim_lib
  _shapes3d_calls(sim_lib(), 'cpu')


@pytest.mark.gpu
def test_shapes3d_neck_issues_the_same_calls_on_the_gpu():
  _shapes3d_calls(_lib.load(), 'cuda:0')


def test_engine_on_the_simulator_matches_the_plain_launches():
  """the neck128 engine of the call-record tests (B = 4) on the simulator: three eager steps, option on and off"""
  from odin_ai_amd.engine import VAEEngine
  from tests.engine_util import case_data, neck_spec
  from tests.simutil import sim_lib
  L = sim_lib()
  spec = neck_spec(4, 128)
  x, eps = case_data('cpu', spec)
  res = []
  for on in (False, True):
    eng = VAEEngine(*spec, 4, 'cpu', lib=L, neck_reduce=on)
    out = []
    for _ in range(3):
      o4 = eng.train_step(x, eps, lr=1e-3, beta=2.0)
      out.append([t.detach().view(torch.int32).clone() for t in (o4, eng.grads, eng.params, eng.m, eng.v)])
    assert eng._bwd_neck() and any(eng._nr_plans.values()) == on
    res.append(out)
  for s in range(3):
    for a, b in zip(res[0][s], res[1][s]):
      assert torch.equal(a, b), ('step', s)


# ---- late jobs that vary from step to step: the label head's job has rows on a labelled step only ---------------------
def _alternating_labels(L, dev):
  """a label_units engine on the neck128 stack, labelled and unlabelled steps in turn: the plan recorded on one kind of
  step serves the other (it reads no rows of a late job), and the steps are those of the plain launches bit for bit"""
  from odin_ai_amd.engine import VAEEngine
  from tests.engine_util import Recorder, case_data, neck_spec
  spec = neck_spec(4, 128)
  x, eps = case_data(dev, spec)
  y = torch.eye(3, device=dev)[[0, 2]].contiguous()
  eps_y = torch.tensor(np.random.default_rng(5).standard_normal((2, 4)), dtype=torch.float32, device=dev)
  res = {}
  for on in (False, True):
    calls = []
    eng = VAEEngine(*spec, 4, dev, lib=Recorder(L, calls), label_units=3, neck_reduce=on)
    out = []
    for lab in (True, False, True, False, False, True):
      eng.train_step(x, eps, lr=1e-3, beta=2.0, labels=y if lab else None, eps_y=eps_y if lab else None)
      out.append([t.detach().view(torch.int32).cpu().clone() for t in (eng.out4, eng.grads, eng.params, eng.m, eng.v)])
    assert eng._bwd_neck()
    # one record serves both kinds of step: every step but the first took the reducing launch
    assert calls.count('odin_neck_bwd_reduce') == (5 if on else 0) and calls.count('odin_label_head_fwd_bwd') >= 3
    res[on] = out
  for s_, (a, b) in enumerate(zip(res[False], res[True])):
    for i, (u, v) in enumerate(zip(a, b)):
      assert torch.equal(u, v), ('step', s_, 'tensor', i)


def test_alternating_labelled_steps_on_the_simulator():
  from tests.simutil import sim_lib
  _alternating_labels(sim_lib(), 'cpu')


@pytest.mark.gpu
def test_alternating_labelled_steps_on_the_gpu():
  _alternating_labels(_lib.load(), 'cuda:0')


# ---- the reducers need idle CUs -------------------------------------------------------------------------------------------
def _query(w, mask=None):
  return w.L.odin_neck_reduce_workgroups(C.byref(w.A), w.jobs, w.n_jobs, w.mask if mask is None else mask, w.g.data_ptr(),
                                         w.g.numel())


def test_too_few_idle_cus_on_the_simulator():
  """the simulator has 16 CUs: the long list (121 virtual blocks) wants 31 reducers beside one neck workgroup -- the
  query says 0 and the launch refuses to pick a count by itself (an explicit count is the caller's business)"""
  from tests.simutil import sim_lib
  L = sim_lib()
  w = World(L, 'cpu', 2, LONG)
  before, _ = w.state()
  assert _query(w) == 0
  with pytest.raises(OdinError, match=r'rc=-2'):
    L.odin_neck_bwd_reduce(C.byref(w.A), w.jobs, w.n_jobs, w.mask, w.g.data_ptr(), w.g.numel(), w.part.data_ptr(), -1, None)
  after, _ = w.state()
  for k in before:
    assert torch.equal(before[k], after[k]), k
  s = World(L, 'cpu', 2, SHORT)
  assert _query(s) == 1 and _query(s, 0) == 0


@pytest.mark.gpu
def test_reducer_count_on_the_gpu():
  w = World(_lib.load(), 'cuda:0', 8, LONG)
  nvb = 5 * 16 + 17 + 3 + 2 + 1 + 128     # (the 4133-float odd job: 130 column blocks on a grid 128 wide)
  assert _query(w) == (nvb + 3) // 4
  assert _query(w, w.mask | (1 << (w.n_jobs - 1))) == 0   # (a mask the launch rejects)


@pytest.mark.gpu
def test_large_batch_keeps_the_plain_launches():
  """B = 512: 256 neck workgroups, one per CU of the part -- no CU is left to a reducer, the engine records that and
  issues the plain launches at every step"""
  from tests.engine_util import Recorder
  calls = []
  eng, x, eps = _dsprites_engine(512, 'cuda:0', lib=Recorder(_lib.load(), calls), neck_reduce=True)
  for _ in range(3):
    eng.train_step(x, eps, lr=1e-3, beta=4.0)
  torch.cuda.synchronize()
  assert eng._bwd_neck() and list(eng._nr_plans.values()) == [False]
  # (odin_slab_reduce_sumsq: the three launches and the first step's dry run for the partial count)
  assert calls.count('odin_neck_bwd') == 3 and calls.count('odin_slab_reduce_sumsq') == 4
  assert 'odin_slab_reduce_sumsq_masked' not in calls
  assert 'odin_neck_bwd_reduce' not in calls and calls.count('odin_neck_reduce_workgroups') == 1
  assert float(eng.grads.abs().max()) > 0 and int(eng.flag.item()) == 0
