"""The sharded training step with W engines in ONE process on the `bk` backend (the CPU simulator, or one MI355X): the
comparison of tests/test_dp_gloo.py and tests/test_latent_reg_dp_gloo.py without processes, gloo or RCCL.  Every engine
is built with world_size = W and a local batch of 8 // W; its `comm` is a loopback object with the interface of
`dist.Comm`; the W launch programs (`VAEEngine.step_program`) are walked in lock step -- segment s of every rank before
segment s + 1 of any -- and at a collective every rank's call posts its tensors, the last one to post performing the
collective on all of them with plain torch ops.  Eager launches only (no graph capture), three steps, against one engine
on the global batch of 8 with the tolerances of the gloo tests."""
import numpy as np
import pytest
import torch

from odin_ai_amd.dist import SegmentedGraph, shard_batch
from odin_ai_amd.engine import VAEEngine
from tests.test_dp_gloo import _data, _init, _spec
from tests.test_latent_reg_dp_gloo import REG

POL = (100.0, None, None, None, True)   # global_clipnorm 100, NaN check: the policy the gloo tests run
STEPS = 3


class Hub:
  """What the W loopback objects share: call k of every rank meets in slot k"""

  def __init__(self, world):
    self.world, self.slots, self.done = world, {}, []

  def post(self, k, rank, op, tensors):
    slot = self.slots.setdefault(k, {})
    assert rank not in slot
    slot[rank] = (op, tensors)
    if len(slot) < self.world:
      return
    del self.slots[k]
    assert {o for o, _ in slot.values()} == {op}, 'the ranks disagree about collective %d' % k
    args = [slot[r][1] for r in range(self.world)]
    getattr(self, op)(args)
    self.done.append(op)

  def all_reduce(self, args):
    tot = args[0][0].clone()
    for (t,) in args[1:]:
      tot += t
    for (t,) in args:
      t.copy_(tot)

  def all_gather(self, args):
    whole = torch.cat([inp.reshape(-1) for _, inp in args])
    for out, _ in args:
      out.view(-1).copy_(whole)

  def reduce_scatter(self, args):
    tot = args[0][1].reshape(-1).clone()
    for _, inp in args[1:]:
      tot += inp.reshape(-1)
    n = args[0][0].numel()
    for r, (out, _) in enumerate(args):
      out.view(-1).copy_(tot[r * n:(r + 1) * n])


class Loopback:
  """`dist.Comm`'s interface (rank, world, all_reduce, all_gather, reduce_scatter) over a Hub"""
  native = False

  def __init__(self, hub, rank):
    self.hub, self.rank, self.world, self.calls = hub, rank, hub.world, 0

  def _post(self, op, *tensors):
    k, self.calls = self.calls, self.calls + 1
    self.hub.post(k, self.rank, op, tensors)

  def all_reduce(self, t):
    self._post('all_reduce', t)

  def all_gather(self, out, inp):
    assert out.numel() == self.world * inp.numel() and out.is_contiguous() and inp.is_contiguous()
    self._post('all_gather', out, inp)

  def reduce_scatter(self, out, inp):
    assert inp.numel() == self.world * out.numel() and out.is_contiguous() and inp.is_contiguous()
    self._post('reduce_scatter', out, inp)

  def close(self):
    pass


def _engine(bk, B, **kw):
  enc, dec, shp, D = _spec()
  eng = VAEEngine(enc, dec, shp, D, B, bk.dev, lib=bk.L, **kw)
  _init(eng)
  return eng


def _sync(bk):
  if bk.dev.type == 'cuda':
    torch.cuda.synchronize()


def run_sharded(bk, W, beta, **kw):
  """three lock-step steps of W engines; returns (engines, out4 of rank 0 per step [STEPS, 4], segment kinds)"""
  x, eps = _data(8)
  x, eps = x.to(bk.dev), eps.to(bk.dev)
  hub = Hub(W)
  per_rank_seed = kw.pop('per_rank_seed', False)
  engs = []
  for r in range(W):
    kr = dict(kw, seed=1 + r) if per_rank_seed else kw
    eng = _engine(bk, 8 // W, world_size=W, **kr)
    eng.comm = Loopback(hub, r)
    engs.append(eng)
  shards = [(shard_batch(x, r, W), shard_batch(eps, r, W)) for r in range(W)]
  outs, kinds = [], None
  for _ in range(STEPS):
    progs = []
    for eng, (xs, es) in zip(engs, shards):
      eng.step_count += 1
      eng.set_hyper(lr=1e-3, beta=beta)
      progs.append(SegmentedGraph(bk.dev, eng.step_program(xs, es, POL)).segs)
    kinds = [''.join(k for k, _ in segs) for segs in progs]
    assert len(set(kinds)) == 1, kinds
    for s in range(len(progs[0])):
      for segs in progs:
        kind, f = segs[s]
        for fn in (f if kind == 'k' else [f]):
          fn()
      assert not hub.slots, 'a collective of segment %d is still waiting for a rank' % s
    _sync(bk)
    outs.append(engs[0].out4.clone())
  assert hub.done and len(hub.done) % STEPS == 0
  return engs, torch.stack(outs), kinds[0]


def run_single(bk, beta, **kw):
  x, eps = _data(8)
  x, eps = x.to(bk.dev), eps.to(bk.dev)
  eng = _engine(bk, 8, **kw)
  outs = []
  for _ in range(STEPS):
    eng.step_count += 1
    eng.set_hyper(lr=1e-3, beta=beta)
    prog = eng.step_program(x, eps, POL)
    assert all(kind == 'k' for kind, _ in prog)
    for _, fn in prog:
      fn()
    _sync(bk)
    outs.append(eng.out4.clone())
  return eng, torch.stack(outs)


def check(engs, eng1, outs, outs1, term):
  # identical maths, different fp32 summation order (per-rank partial sums): the bounds of tests/test_dp_gloo.py
  d = (eng1.params - engs[0].params).abs()
  assert d.max().item() < 2e-4 and d.mean().item() < 2e-6, (d.max().item(), d.mean().item())
  for e in engs[1:]:   # replicas stay replicas
    assert torch.equal(e.params, engs[0].params)
  assert bool(torch.isfinite(outs).all())
  if term:
    # out4[0:3] are rank 0's local means; the TC / regulariser term is the global batch's on every rank
    for got, want in zip(outs[:, 3].tolist(), outs1[:, 3].tolist()):
      assert abs(want) > 0 and abs(got - want) <= 1e-4 * max(1.0, abs(want)), (got, want)
    for e in engs[1:]:
      assert abs(e.out4[3].item() - engs[0].out4[3].item()) <= 1e-4 * max(1.0, abs(engs[0].out4[3].item()))


@pytest.mark.parametrize('W', [2, 4])
def test_plain_step(bk, W):
  """two gradient buckets: the decoder's reduced before the encoder's backward pass ends (on a GPU: on each engine's side
  stream, joined before the update, which the loopback's torch ops follow like any other work on those streams)"""
  engs, outs, kinds = run_sharded(bk, W, 4.0, dp_buckets=2)
  assert kinds == 'kckck', kinds
  eng1, outs1 = run_single(bk, 4.0)
  check(engs, eng1, outs, outs1, term=False)


@pytest.mark.parametrize('buckets,kinds', [(1, 'kckckck'), (2, 'kckckckck')])
def test_beta_tc_step(bk, buckets, kinds):
  """all-gather of (p, z) | odin_total_correlation_shard | reduce-scatter of the posterior-side planes + all-reduce of
  the value | backward | gradient all-reduce(s) | update, with B_local = 4 of B_global = 8"""
  engs, outs, got = run_sharded(bk, 2, 4.0, tc='betatc', dp_buckets=buckets)
  assert got == kinds, got
  eng1, outs1 = run_single(bk, 4.0, tc='betatc')
  check(engs, eng1, outs, outs1, term=True)


@pytest.mark.parametrize('reg,kinds', [('mmd', 'kckckck'), ('dip_ii', 'kckck')])
def test_latent_regulariser_step(bk, reg, kinds):
  """MMD: all-gather z | odin_mmd_shard (k(y, y) on rank 0, the prior drawn in the launch from the shared prior seed) |
  all-reduce of the shares; DIP-II: odin_dip_moments | all-gather of the blocks | odin_dip_finish.  Each rank its own
  engine seed, the prior seed shared, as tests/test_latent_reg_dp_gloo.py builds them; one gradient bucket (the two-bucket
  split is the same code whatever the regulariser: test_plain_step, test_beta_tc_step)."""
  engs, outs, got = run_sharded(bk, 2, 2.0, per_rank_seed=True, dp_buckets=1, prior_seed=3, **REG[reg])
  assert got == kinds, got
  eng1, outs1 = run_single(bk, 2.0, prior_seed=3, **REG[reg])
  check(engs, eng1, outs, outs1, term=True)
