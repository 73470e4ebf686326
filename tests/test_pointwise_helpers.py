"""The small C-ABI helpers of pointwise.hip / tc.hip -- odin_logmeanexp_rows, odin_sum_parts, odin_mean and the two
batch gathers -- against float64 / numpy references, outputs inside guard bands.  Fixture `bk`: simulator and hipcc."""
import numpy as np
import pytest
import torch

from oracle import data_oracle as do
from tests.adam_util import F32, F64, Guard, ptr
from tests.test_pointwise import close


@pytest.mark.parametrize('kind', ['ordinary', 'deep'])
@pytest.mark.parametrize('n,B', [(1, 1), (7, 255), (100, 256), (3, 257), (1000, 5)])
def test_logmeanexp_rows(bk, n, B, kind):
  """out[b] = log mean_k exp(in[k][b]) against float64 on the float32-rounded input; 'deep': values near -3000 with a
  spread of 200 (exp underflows for all but the column maximum); columns 0..2 (where there are that many): all equal,
  some -inf (finite result), all -inf (-inf, not NaN)"""
  rng = np.random.default_rng(n + B)
  x = (rng.standard_normal((n, B)) * 3.0 if kind == 'ordinary' else -3000.0 + 200.0 * rng.random((n, B))).astype(F32)
  special = B >= 3 and n >= 2
  if special:
    x[:, 0] = x[0, 0]
    x[::2, 1] = -np.inf
    x[:, 2] = -np.inf
  G = Guard(bk)
  tx, out = G.buf('in', x, frozen=True), G.buf('out', np.zeros(B))
  bk.L.odin_logmeanexp_rows(ptr(tx), ptr(out), n, B, None)
  G.check()
  x64 = x.astype(F64)
  with np.errstate(all='ignore'):
    mx = x64.max(0)
    ref = np.where(np.isfinite(mx), mx + np.log(np.exp(x64 - np.where(np.isfinite(mx), mx, 0.0)).sum(0)), -np.inf) - np.log(n)
  got = out.cpu().numpy()
  fin = np.isfinite(ref)
  assert fin.sum() == B - (1 if special else 0)
  assert np.array_equal(got[~fin], ref[~fin])   # -inf exactly
  close(got[fin], ref[fin], 2e-5)
  if special:
    close(got[:1], x64[:1, 0], 2e-5)            # the mean of n equal values


@pytest.mark.parametrize('B,n_part', [(1, 1), (5, 7), (256, 8), (257, 9), (9, 100), (300, 240)])
def test_sum_parts(bk, B, n_part):
  rng = np.random.default_rng(B + n_part)
  part = (rng.standard_normal((B, n_part)) * 30).astype(F32)
  G = Guard(bk)
  tp, out = G.buf('part', part, frozen=True), G.buf('out', np.zeros(B))
  bk.L.odin_sum_parts(ptr(tp), n_part, ptr(out), B, None)
  G.check()
  close(out.cpu().numpy(), part.astype(F64).sum(1), 1e-5)


@pytest.mark.parametrize('n', [1, 63, 64, 255, 256, 257, 5000])
def test_mean(bk, n):
  """against float64.  A thread chains ceil(n / 256) <= 20 additions, the wave and block trees add 8, the division
  one rounding: |error| <= 29 * 2^-24 * mean |x| = 1.7e-6 * mean |x| for any signs; the bound asserted is 2e-6"""
  x = (np.random.default_rng(n).standard_normal(n) * 3.0 + 0.5).astype(F32)
  G = Guard(bk)
  tx, out = G.buf('x', x, frozen=True), G.buf('out', np.zeros(1))
  bk.L.odin_mean(ptr(tx), n, ptr(out), None)
  G.check()
  x64 = x.astype(F64)
  assert abs(out.item() - x64.mean()) <= 2e-6 * np.abs(x64).mean()


@pytest.mark.parametrize('n_per', [4, 12, 4096])
@pytest.mark.parametrize('B', [1, 3, 300])
def test_gather_rows_f32(bk, B, n_per):
  """out[b] = data[idx[b]] bit for bit: repeated and descending indices, idx an int32 offset into a longer
  permutation (as fit() passes it)"""
  N, off = 17, 5
  rng = np.random.default_rng(B * n_per)
  data = rng.standard_normal((N, n_per)).astype(F32)
  perm = np.concatenate([rng.integers(0, N, off), np.arange(B)[::-1] % N, rng.integers(0, N, 3)]).astype(np.int32)
  if B >= 3:
    perm[off + 1] = perm[off]   # a repeated row
  G = Guard(bk)
  td, tp = G.buf('data', data, frozen=True), G.buf('perm', perm, torch.int32, frozen=True)
  out = G.buf('out', np.zeros(B * n_per))
  bk.L.odin_gather_rows_f32(ptr(td), ptr(tp, off), ptr(out), B, n_per, None)
  G.check()
  ref = bk.T(data[perm[off:off + B]].reshape(-1))
  assert torch.equal(out.view(torch.int32), ref.view(torch.int32))


def test_gather_rows_f32_rejects_ragged_rows(bk):
  G = Guard(bk)
  td = G.buf('data', np.arange(30.0))
  tp, out = G.buf('idx', np.array([1, 0]), torch.int32), G.buf('out', np.full(12, 3.0))
  G.freeze()
  assert bk.L.c.odin_gather_rows_f32(ptr(td), ptr(tp), ptr(out), 2, 6, None) == -2
  assert len(bk.L.c.odin_last_error()) > 0
  G.check()


MODES = ['probs', 'tanh', 'raster', 'binarized']


@pytest.mark.parametrize('n_per', [16, 64 * 64])
@pytest.mark.parametrize('premul', [1.0, 255.0])
@pytest.mark.parametrize('mode', MODES)
def test_gather_normalize_u8(bk, mode, premul, n_per):
  """uint8 gather + ImageDataset.normalize, every byte value in the input: bit-exact against oracle/data_oracle.py,
  and against the float64 formula"""
  N = 20 if n_per == 16 else 3
  rng = np.random.default_rng(n_per)
  imgs = rng.permutation(np.arange(N * n_per) % 256).astype(np.uint8).reshape(N, n_per)
  assert len(np.unique(imgs)) == 256
  idx = np.array([N - 1, 0, 2, 2, 1], np.int32)
  B = len(idx)
  G = Guard(bk)
  td, ti = G.buf('data', imgs, torch.uint8, frozen=True), G.buf('idx', idx, torch.int32, frozen=True)
  out = G.buf('out', np.zeros(B * n_per))
  bk.L.odin_gather_normalize_u8(ptr(td), ptr(ti), ptr(out), B, n_per, premul, do.MODES[mode], None)
  G.check()
  got = out.cpu().numpy().reshape(B, n_per)
  assert np.array_equal(got, do.gather_normalize(imgs, idx, mode, premul))
  x = imgs[idx].astype(F64) * premul
  if mode != 'binarized':
    x = np.clip(x, 0.0, 255.0)
  if mode == 'probs':
    x = np.clip(x / 255.0, 1e-6, 1.0 - 1e-6)
  elif mode == 'tanh':
    x = np.clip(x / 255.0 * 2.0 - 1.0, -1.0 + 1e-6, 1.0 - 1e-6)
  close(got, x, 1e-7)


@pytest.mark.parametrize('n_per,mode', [(24, 0), (16, 4)])
def test_gather_normalize_u8_rejects(bk, n_per, mode):
  G = Guard(bk)
  td = G.buf('data', np.arange(96) % 256, torch.uint8)
  ti, out = G.buf('idx', np.array([1, 0]), torch.int32), G.buf('out', np.full(48, 3.0))
  G.freeze()
  assert bk.L.c.odin_gather_normalize_u8(ptr(td), ptr(ti), ptr(out), 2, n_per, 1.0, mode, None) == -2
  assert len(bk.L.c.odin_last_error()) > 0
  G.check()
