"""Which kernel family serves which layer, against tests/golden/dispatch_table.json (recorded by tests/dispatch_util.py
before the dispatch chains were folded into one selector per op): the row counts of every dry run, the answers of the
*_keeps_range / *_reads_x_range predicates and the kernel each op launches, for every layer of the benchmark networks
and a list of edge cases, once more under ODIN_EXACT_FP32.  The record holds the simulator's keys (`sim`, `sim_paths`:
16 compute units, launches of a dozen smallest shapes) and the GPU's (`hip`, `hip_paths`: the device's compute units, one
launch per op of every case at its real shape on zero-filled buffers); each test asserts equality with its own."""
import json

import pytest

from tests import dispatch_util as du


@pytest.fixture(scope='module')
def golden():
  with open(du.GOLDEN) as f:
    return json.load(f)


def _compare(got, golden):
  assert got, 'nothing was recorded'
  for key, table in got.items():
    assert key in golden, 'no record under %r in %s' % (key, du.GOLDEN)
    assert sorted(table) == sorted(golden[key]), key
    bad = {c: (table[c], golden[key][c]) for c in table if table[c] != golden[key][c]}
    assert not bad, (key, bad)


def test_dispatch_table_on_the_simulator(golden):
  from tests.simutil import sim_lib
  _compare(du.record(sim_lib(), 'cpu', 'sim'), golden)


@pytest.mark.gpu
def test_dispatch_table_on_the_gpu(golden):
  from odin_ai_amd import _lib
  _compare(du.record(_lib.load(), 'cuda:0', 'hip'), golden)

