"""The launches that close a training step -- the five flat Adam launchers of pointwise.hip, all driving adam_kernel --
against the float64 oracle (vo.adam_keras / vo.clip_by_global_norm), bit for bit against each other, with the hyper
ring, the ELBO finalisation that rides in an extra workgroup and the fused second stage of the gradient norm; every
buffer sits inside guard bands (tests/adam_util.py).  Fixture `bk`: the CPU simulator build and the hipcc build."""
import math

import numpy as np
import pytest

from odin_ai_amd.engine import N_HYPER
from tests import adam_util as au
from tests.adam_util import F32, F64, LAYOUTS, LAUNCHERS, Harness, Rows, ptr
from tests.test_pointwise import close

SMALL = (1, 3, 4, 5, 1020, 1023, 1024, 1027)
# past the stage-1 cap of 1024 workgroups / past Adam's cap of 2048: every thread walks its grid-stride loop twice
LARGE = (2 ** 20 + 2 ** 18 + 1, 3 * 2 ** 20 + 7)
MATRIX = [(n, mode, la) for n in SMALL + LARGE for mode in ('off', 'active', 'inactive') for la in LAUNCHERS]


def skip_large_on_sim(bk, n):
  if bk.name == 'sim' and n in LARGE:
    pytest.skip('large shapes run on the GPU backend only (fiber simulator: minutes)')


@pytest.mark.parametrize('n,mode,launcher', MATRIX)
def test_flat_launchers(bk, n, mode, launcher):
  """launcher x size x clip: theta, m, v against the oracle, the norm against the float64 sum, bit identity with
  odin_adam_step_flat (and odin_sumsq_flat / odin_sumsq_adam_flat), guard bands, g and the ring unchanged"""
  skip_large_on_sim(bk, n)
  th, g, m, v, g2 = au.base(n)
  h = Harness(bk, th, g, m, v, fin=(5, 1) if n & 1 else (70, 33), tc=bool(n & 2))
  h.step(launcher, au.clip_for(mode, g2), g2, ref=au.matrix_oracle(n, mode))


@pytest.mark.parametrize('n_parts', [1, 255, 256, 257, 2048])
@pytest.mark.parametrize('mode', ['off', 'active'])
def test_ring_parts_sums_any_number_of_partials(bk, n_parts, mode):
  """the fused second stage of the norm over hand-made non-negative partials: gnorm2_out against their float64 sum
  (<= 8 chained additions per thread + the block tree: within the 1e-5 of the norm), the clip scale follows it"""
  n = 1027
  th, g, m, v, _ = au.base(n)
  parts = (np.random.default_rng(n_parts).random(n_parts) * 3.0).astype(F32)
  s = float(parts.astype(F64).sum())
  clip = au.clip_for(mode, s)
  h = Harness(bk, th, g, m, v, no_ring=True)
  tp = h.G.buf('parts', parts, frozen=True)
  _, sc, lr, _, _ = h.table(h.t)
  h.launch('ring_parts', clip, keep_parts=True, parts=ptr(tp), n_parts=n_parts)
  h.G.check()
  assert abs(h.gn.item() - s) <= 1e-5 * s and h.flag.item() == 0
  # the oracle clips by the norm it is given: scale the gradient so that its own norm is sqrt(s)
  gsc = np.asarray(g, F64)
  if clip > 0:
    gsc = gsc * (clip / max(math.sqrt(s), clip))
  ref = au.oracle_update(th, gsc, m, v, h.t, lr, sc, 0.0)
  for got, want in zip((h.th, h.m, h.v), ref):
    close(got.cpu().numpy(), want, 1e-6)


@pytest.mark.parametrize('launcher', LAUNCHERS)
@pytest.mark.parametrize('bad', [np.inf, np.nan])
@pytest.mark.parametrize('where', ['first', 'tail', 'last'])
@pytest.mark.parametrize('flag', [True, False])
def test_non_finite_gradient(bk, launcher, bad, where, flag):
  """one inf / nan in the first element, the first of the ragged tail or the last element.  With a flag: raised,
  theta / m / v bit-unchanged, and the ring variants have STILL advanced `cur` and staged this step's scalars (the
  host's ring bookkeeping counts every step).  Without one, clip off: the update is applied whatever the gradient
  holds -- finite elements match the oracle, the others are non-finite."""
  n = 1027
  th, g, m, v, _ = au.base(n)
  g = g.copy()
  i = {'first': 0, 'tail': (n // 4) * 4, 'last': n - 1}[where]
  g[i] = bad
  h = Harness(bk, th, g, m, v, flag=flag, fin=(9, 100), tc=True)
  finite = np.isfinite(g)
  h.step(launcher, 0.0 if not flag else 2.0, float('nan'), skipped=flag, finite=None if flag else finite)


# ------------------------------------------------------------------------------------------------ the ring ---------
@pytest.mark.parametrize('rows', [2, 8, 16])
@pytest.mark.parametrize('rf', [5, N_HYPER + 4, 24, 64])
@pytest.mark.parametrize('launcher', ['ring', 'ring_parts'])
def test_ring_advance_one_call(bk, launcher, rows, rf):
  """`cur` = ring row (t + 1) mod rows bit for bit, staged[0:5] = the old scalars, the update used the OLD scalars
  (the next row's learning rate is 100 x larger)"""
  n = 1027
  th, g, m, v, g2 = au.base(n)
  for t0 in (6, rows - 1):   # (rows - 1: the slot index wraps)
    h = Harness(bk, th, g, m, v, lay=LAYOUTS[rf], rows=rows, t0=t0, table=Rows(LAYOUTS[rf], seed=rows))
    assert h.table(t0 + 1)[2] > 50 * h.table(t0)[2] or h.table(t0)[2] > 50 * h.table(t0 + 1)[2]
    h.step(launcher, au.clip_for('active', g2), g2)


@pytest.mark.parametrize('B,n_part', [(5, 1), (70, 33), (9, 100)])
@pytest.mark.parametrize('tc', [False, True])
@pytest.mark.parametrize('launcher', ['ring+fin', 'ring_parts+fin', 'finalize_flat'])
@pytest.mark.parametrize('n', [5, 1027])
def test_elbo_finalize_rides_along(bk, launcher, n, tc, B, n_part):
  """the ELBO finalisation in the extra last workgroup: out4 / llk bit-equal to a stand-alone odin_elbo_finalize with
  THIS step's beta and TC weight (elbo_hyper points into `cur`, which the same call advances to a row whose beta
  differs 10 x; odin_adam_ring_parts reads them from the staged row), and against the float64 reference"""
  th, g, m, v, g2 = au.base(n)
  lay = LAYOUTS[24]
  h = Harness(bk, th, g, m, v, lay=lay, rows=8, t0=7, table=Rows(lay, seed=3), fin=(B, n_part), tc=tc)
  assert h.table(7)[3] > 4 * h.table(8)[3]
  h.step(launcher, au.clip_for('inactive', g2), g2)


@pytest.mark.parametrize('rows,rf', [(2, 24), (8, N_HYPER + 4), (16, 64), (8, 5)])
@pytest.mark.parametrize('launcher', ['ring+fin', 'ring_parts+fin', 'ring_parts-noring'])
def test_ring_run_of_steps(bk, launcher, rows, rf):
  """rows + 3 consecutive calls from t = 2 rows - 2 (slot rows - 2, as t = rows - 2 would be, with a step number Adam
  accepts for rows = 2: the slot index wraps after two calls; the host refills the slots behind the kernel as the
  engine does): after every call theta / m / v against the float64 oracle stepped freely with the same
  per-step values (11..19 steps of at most one float32 rounding of theta each: inside close(1e-6) of max |theta|),
  t read back from `cur`; ring = NULL to odin_adam_ring_parts leaves `cur` bit-unchanged"""
  n = 1027
  th, g, m, v, g2 = au.base(n)
  lay, t0 = LAYOUTS[rf], 2 * rows - 2
  no_ring = launcher.endswith('-noring')
  la = 'ring_parts' if no_ring else launcher
  h = Harness(bk, th, g, m, v, lay=lay, rows=rows, t0=t0, table=Rows(lay, seed=rows + rf), fin=(5, 1), tc=True,
              no_ring=no_ring)
  clip = au.clip_for('active', g2)
  ref = tuple(np.asarray(a, F64) for a in (th, m, v))
  for _ in range(rows + 3):
    _, sc, lr, _, _ = h.table(h.t)
    ref = au.oracle_update(ref[0], g, ref[1], ref[2], h.t, lr, sc, clip)
    h.step(la, clip, g2, ref=ref)


BAD_RING = [dict(rows=1), dict(rows=3), dict(rows=12), dict(row_floats=0), dict(row_floats=65), dict(t_word=24),
            dict(cur=None), dict(staged=None)]


@pytest.mark.parametrize('launcher,bad', [('ring', dict(ring=None))] + [('ring', b) for b in BAD_RING] +
                         [('ring_parts', b) for b in BAD_RING] + [('ring_parts', dict(n_parts=0))],
                         ids=lambda x: x if isinstance(x, str) else '-'.join(f'{k}={v}' for k, v in x.items()))
def test_rejected_ring_arguments(bk, launcher, bad):
  """-2, every buffer bit-unchanged, a message in odin_last_error"""
  n = 1027
  th, g, m, v, g2 = au.base(n)
  lay = LAYOUTS[24]
  h = Harness(bk, th, g, m, v, lay=lay, fin=(5, 1), tc=True, table=Rows(lay, seed=1))
  rc = h.launch(launcher + '+fin', 1.0, raw=True, **bad)
  assert rc == -2
  assert len(bk.L.c.odin_last_error()) > 0
  h.G.check()
