"""The entry points that exist only for data parallelism, with ONE process playing every rank in turn on the `bk`
backend (the CPU simulator under `-m "not gpu"`, the gfx950 build under `-m gpu`): a global batch is split into W
contiguous shards as `dist.shard_batch` splits it, the shard entry point runs once per rank, the host combines the
results the way the collectives would, and the outcome is held to the float64 oracle of the GLOBAL batch and to the
fused single-device entry point -- so every `B_local < B_global` distinction (zT[l*Bj + j] against muT[l*Bi + i], the
workspace layout, nt_rows(Bi) against nt_cols(Bj), the `r - Bl` row of the k(y, y) workgroups, grids of Bl + M and of
Bl arrivals) runs without a second device.  Tolerances are those of the tests of the fused forms
(tests/test_pointwise.py, tests/test_latent_regularizers.py), imported from there, not restated.

Also here: the on-device random permutations beyond one trip of their 256-thread loop, and the total-correlation rows
kernel at and just past its LDS limit."""
import functools

import numpy as np
import pytest
import torch

from odin_ai_amd import _lib
from oracle import vae_oracle as vo
from tests.test_latent_regularizers import _st, assert_grad, assert_value, np_dip, np_mmd, np_mmd_grad
from tests.test_pointwise import close

SENTINEL = -12345.5
GUARD = 256


def _frozen(*arrays):
  for a in arrays:
    a.setflags(write=False)
  return arrays


# ---- total correlation ----------------------------------------------------------------------------------------------
def tc_oracle_blocked(z, loc, scale, rows=64):
  """vo.total_correlation and vo.total_correlation_bwd, the [j, i, l] intermediates formed `rows` values of j at a time"""
  B = z.shape[0]
  tc, gz, gl, gs = 0.0, np.zeros_like(z), np.zeros_like(loc), np.zeros_like(scale)
  for j0 in range(0, B, rows):
    zj = z[j0:j0 + rows]
    d = (zj[:, None, :] - loc[None, :, :]) / scale[None, :, :]
    lp = -0.5 * d ** 2 - np.log(scale[None, :, :]) - 0.5 * vo.LOG2PI
    s = lp.sum(2)
    lse_l, lse_j = vo._logsumexp(lp, 1), vo._logsumexp(s, 1)
    tc += float((lse_j - lse_l.sum(1)).sum())
    g = (np.exp(s - lse_j[:, None])[:, :, None] - np.exp(lp - lse_l[:, None, :])) / B
    gz[j0:j0 + rows] = (g * (-d / scale[None])).sum(1)
    gl += (g * (d / scale[None])).sum(0)
    gs += (g * ((d ** 2 - 1.0) / scale[None])).sum(0)
  return tc / B, gz, gl, gs


@functools.lru_cache(maxsize=None)
def tc_case(B, D, spread, blocked=False):
  """inputs in the regime the step is in (z a sample of its own posterior, as test_total_correlation_on_posterior_samples
  draws them) and the float64 oracle of the whole batch; computed once per size, read-only"""
  rng = np.random.default_rng(6)
  p = rng.standard_normal((B, 2 * D)) * spread
  loc, sc = vo.mvn_diag_params(p.astype(np.float32).astype(np.float64), D)
  z = (loc + sc * rng.standard_normal((B, D))).astype(np.float32).astype(np.float64)
  if blocked:
    tc_ref, gz, gl, gs = tc_oracle_blocked(z, loc, sc)
  else:
    tc_ref = vo.total_correlation(z, loc, sc)
    gz, gl, gs = vo.total_correlation_bwd(z, loc, sc)
  return (tc_ref,) + _frozen(p, z, gz, gl, gs)


def test_blocked_tc_oracle_is_the_oracle():
  tc_ref, p, z, gz, gl, gs = tc_case(70, 6, 1.0)
  loc, sc = vo.mvn_diag_params(p.astype(np.float32).astype(np.float64), 6)
  tc_b, gz_b, gl_b, gs_b = tc_oracle_blocked(z, loc, sc, rows=16)   # (70 = 4 x 16 + 6: a ragged last block)
  assert abs(tc_b - tc_ref) <= 1e-12 * max(1.0, abs(tc_ref))
  for a, b in ((gz_b, gz), (gl_b, gl), (gs_b, gs)):
    assert np.abs(a - b).max() <= 1e-12 * np.abs(b).max()


def tc_fused(bk, p, z, coef, B, D):
  L = bk.L
  tz, tp, tcf = bk.T(z), bk.T(p), bk.T([coef])
  ws = bk.zeros(L.odin_total_correlation_workspace(B, B, D))
  dz, dl, ds = bk.zeros(B, D), bk.zeros(B, D), bk.zeros(B, D)
  L.odin_total_correlation_fwd_bwd(tz.data_ptr(), tp.data_ptr(), ws.data_ptr(), dz.data_ptr(), dl.data_ptr(),
                                   ds.data_ptr(), tcf.data_ptr(), B, D, _st(bk.dev))
  return ws, dz, dl, ds


def rel_to_max(got, ref):
  return np.abs(np.asarray(got, np.float64) - ref).max() / np.abs(ref).max()


TC_SHAPES = [(2, 70, 6),       # Bl = 35: ragged against 64 lanes
             (8, 24, 10),      # Bl = 3
             (4, 4, 5),        # Bl = 1
             (2, 256, 10),     # nt_rows 512 over nt_cols 256
             (2, 512, 8),      # 1024 over 512
             (8, 512, 45)]     # CelebA beta-TCVAE at 64 per rank: 92 KB of LDS, 1024-thread rows, 256-thread columns
TC_HIP_ONLY = {(8, 512, 45)}


@pytest.mark.parametrize('spread', [1.0, 0.3])
@pytest.mark.parametrize('W,Bg,D', TC_SHAPES)
def test_total_correlation_shards(bk, W, Bg, D, spread):
  if bk.name == 'sim' and (W, Bg, D) in TC_HIP_ONLY:
    pytest.skip('large shapes run on the GPU backend only (fiber simulator: minutes)')
  L, coef, Bl = bk.L, 3.0, Bg // W
  tc_ref, p, z, gz, gl, gs = tc_case(Bg, D, spread)
  _, dz_fused, _, _ = tc_fused(bk, p, z, coef, Bg, D)
  tp, tz, tcf = bk.T(p), bk.T(z), bk.T([coef])
  n_ws = L.odin_total_correlation_workspace(Bl, Bg, D)
  # the buffer behind the workspace is as long as the single-device workspace (never shorter than a shard's) plus
  # the guard, so a launch that outruns the size the library reports lands in the sentinel, not past the allocation
  n_buf = L.odin_total_correlation_workspace(Bg, Bg, D) + GUARD
  assert n_ws + GUARD <= n_buf
  shares, dz_rows, dl_parts, ds_parts = [], [], [], []
  for r in range(W):
    buf = bk.full((n_buf,), SENTINEL)
    buf[:n_ws] = 0.0
    dz = bk.full((Bl, D), float('nan'))
    dl, ds = bk.full((Bg, D), float('nan')), bk.full((Bg, D), float('nan'))
    L.odin_total_correlation_shard(tz[r * Bl:].data_ptr(), tp.data_ptr(), buf.data_ptr(), dz.data_ptr(), dl.data_ptr(),
                                   ds.data_ptr(), tcf.data_ptr(), Bl, Bg, D, _st(bk.dev))
    assert bool((buf[n_ws:] == SENTINEL).all()), 'a write past odin_total_correlation_workspace(Bl, Bg, D) floats'
    # every posterior row is written by every rank
    assert bool(torch.isfinite(dz).all()) and bool(torch.isfinite(dl).all()) and bool(torch.isfinite(ds).all())
    # tc_rows_kernel runs the same arithmetic for a row whichever launch it sits in (the same B = Bi, the same nt_rows)
    assert torch.equal(dz, dz_fused[r * Bl:(r + 1) * Bl]), r
    shares.append(float(buf[0]))
    dz_rows.append(dz)
    dl_parts.append(dl)
    ds_parts.append(ds)
  close([sum(shares)], [tc_ref], 1e-5)
  # concatenation = all rows of dz; fp32 sums over ranks = what reduce-scatter forms
  got = dict(dz=torch.cat(dz_rows), dloc=torch.stack(dl_parts).sum(0), dscale=torch.stack(ds_parts).sum(0))
  for nm, ref in (('dz', gz), ('dloc', gl), ('dscale', gs)):
    e = rel_to_max(got[nm].cpu().numpy(), coef * ref)
    assert e <= 1e-4, (nm, e)


def test_total_correlation_near_the_lds_limit(bk):
  """B = 1024, D = 36: (B*D + 2B + 2D + 8) * 4 = 155 968 B of the 161 792 B of dynamic LDS the rows kernel may ask for
  (the largest size otherwise tested uses 92 KB)"""
  if bk.name == 'sim':
    pytest.skip('large shapes run on the GPU backend only (fiber simulator: minutes)')
  B, D, coef = 1024, 36, 3.0
  tc_ref, p, z, gz, gl, gs = tc_case(B, D, 1.0, blocked=True)
  ws, dz, dl, ds = tc_fused(bk, p, z, coef, B, D)
  close([ws[0].item()], [tc_ref], 1e-5)
  for got, ref, nm in ((dz, gz, 'dz'), (dl, gl, 'dloc'), (ds, gs, 'dscale')):
    e = rel_to_max(got.cpu().numpy(), coef * ref)
    assert e <= 1e-4, (nm, e)


def test_total_correlation_past_the_lds_limit_is_an_error(bk):
  """B = 2048, D = 18 asks for 164 016 B: refused through the library's error path before any launch"""
  if bk.name == 'sim':
    pytest.skip('large shapes run on the GPU backend only (fiber simulator: minutes)')
  L, B, D = bk.L, 2048, 18
  rng = np.random.default_rng(2)
  tz, tp, tcf = bk.T(rng.standard_normal((B, D))), bk.T(rng.standard_normal((B, 2 * D))), bk.T([3.0])
  ws = bk.full((L.odin_total_correlation_workspace(B, B, D),), float('nan'))
  dz, dl, ds = (bk.full((B, D), float('nan')) for _ in range(3))
  with pytest.raises(_lib.OdinError, match='too large for LDS'):
    L.odin_total_correlation_fwd_bwd(tz.data_ptr(), tp.data_ptr(), ws.data_ptr(), dz.data_ptr(), dl.data_ptr(),
                                     ds.data_ptr(), tcf.data_ptr(), B, D, _st(bk.dev))
  for t in (ws, dz, dl, ds):
    assert bool(torch.isnan(t).all())


# ---- MMD ------------------------------------------------------------------------------------------------------------
MMD_SHAPES = [
    # (W, Bg, D, M), the same on the simulator unless a smaller (Bg, M) is named: there Bg (Bg + M) D <= 2 000 000
    ((2, 20, 6, 37), None),       # M D and row starts that are no multiples of 4 in the Philox stream
    ((4, 8, 3, 5), None),
    ((8, 8, 1, 1), None),         # Bl = 1, D = 1
    # D = 64 stages 128 rows per chunk: x_all and y span several chunks with a ragged last one (simulator: x_all
    # spans two chunks, 128 + 4 rows; 132 * 232 * 64 = 1 959 936)
    ((2, 260, 64, 130), (132, 100)),
    ((8, 512, 10, 512), 'hip'),
]
KIND = {'gaussian': 0, 'linear': 1}


@functools.lru_cache(maxsize=None)
def mmd_case(Bg, D, M):
  rng = np.random.default_rng(Bg + D + M)
  x = (rng.standard_normal((Bg, D)) * 0.8 + 0.3).astype(np.float32)
  y = rng.standard_normal((M, D)).astype(np.float32)
  return _frozen(x, y)


def mmd_shard_run(bk, ws, xt, yt, kernel, W, M, cf, cg, yy_rank, seed=0, step=None, grad=True, ranks=None):
  """every rank's launch in turn on the ONE workspace `ws` (zeroed by the caller once, never again); returns the value
  shares and the dz_local of every rank"""
  Bg, D = xt.shape
  Bl = Bg // W
  shares, dzs = [], []
  for r in (range(W) if ranks is None else ranks):
    dz = bk.full((Bl, D), float('nan')) if grad else None
    bk.L.odin_mmd_shard(xt[r * Bl:].data_ptr(), xt.data_ptr(), yt.data_ptr() if yt is not None else None, ws.data_ptr(),
                        dz.data_ptr() if grad else None, cf.data_ptr(), cg.data_ptr(), Bl, Bg, M, D, KIND[kernel],
                        int(r == yy_rank), seed, step.data_ptr() if step is not None else None, _st(bk.dev))
    shares.append(ws[:1].clone())
    # the last arrival of the launch (of Bl + M workgroups on the k(y, y) rank, of Bl elsewhere) cleared the accumulator
    assert int(ws[2:].view(torch.int32).abs().sum()) == 0, (r, yy_rank)
    dzs.append(dz)
  return shares, dzs


def total(shares):
  return sum(float(s[0]) for s in shares)


@pytest.mark.parametrize('kernel', ['gaussian', 'linear'])
@pytest.mark.parametrize('shape,sim', MMD_SHAPES, ids=['-'.join(map(str, s)) for s, _ in MMD_SHAPES])
def test_mmd_shards(bk, kernel, shape, sim):
  W, Bg, D, M = shape
  if bk.name == 'sim' and sim == 'hip':
    pytest.skip('large shapes run on the GPU backend only (fiber simulator: minutes)')
  if bk.name == 'sim' and sim is not None:
    Bg, M = sim
  assert bk.name != 'sim' or Bg * (Bg + M) * D <= 2_000_000
  L, Bl, coef, cgrad = bk.L, Bg // W, 2.5, -1.5
  x, y = mmd_case(Bg, D, M)
  xt, yt, cf, cg = bk.T(x), bk.T(y), bk.T([coef]), bk.T([cgrad])
  ws_f, dz_f = bk.zeros(L.odin_mmd_workspace(Bg, Bg, M, D)), bk.zeros(Bg, D)
  L.odin_mmd_fwd_bwd(xt.data_ptr(), yt.data_ptr(), ws_f.data_ptr(), dz_f.data_ptr(), cf.data_ptr(), cg.data_ptr(), Bg, M,
                     D, KIND[kernel], 0, None, _st(bk.dev))
  ref, gref = np_mmd(x, y, kernel), np_mmd_grad(x, y, kernel)
  ws = bk.zeros(L.odin_mmd_workspace(Bl, Bg, M, D))   # zeroed ONCE for every launch of this test
  # -- explicit y, the k(y, y) term on the first rank, then on the last
  totals, all_shares = [], []
  for yy_rank in (0, W - 1):
    shares, dzs = mmd_shard_run(bk, ws, xt, yt, kernel, W, M, cf, cg, yy_rank)
    assert_value(total(shares) / coef, ref)
    assert_grad(torch.cat(dzs).cpu().numpy() / cgrad, gref)
    for r in range(W):   # a row meets the same staged chunks of x_all in either launch
      assert torch.equal(dzs[r], dz_f[r * Bl:(r + 1) * Bl]), (r, yy_rank)
    # forward only (dz = NULL) on the k(y, y) rank: the same share, bit for bit
    fwd, _ = mmd_shard_run(bk, ws, xt, yt, kernel, W, M, cf, cg, yy_rank, grad=False, ranks=[yy_rank])
    assert torch.equal(fwd[0], shares[yy_rank])
    totals.append(total(shares))
    all_shares += shares
  # The workgroups' fixed-point words are the same whichever rank runs the k(y, y) rows, and integer sums do not depend
  # on grouping; what differs is where the float32 roundings of the shares fall: each share is off by at most 2^-24 of
  # itself (the float64 product before it: 2^-52), so the two totals differ by at most 2^-24 (1 + 2^-20) sum |share|.
  assert abs(totals[0] - totals[1]) <= 2.0 ** -24 * (1 + 2.0 ** -20) * sum(abs(float(s[0])) for s in all_shares)
  # -- y = NULL: the prior sample drawn inside the launch, the same (prior_seed, step) on every rank, against the explicit-y
  # run on the first M D elements of the stream odin_rng_normal(prior_seed, step) writes
  step, seed = bk.T(np.array([7], np.int32), torch.int32), 12345 | (3 << 32)
  yp = bk.zeros(M, D)
  L.odin_rng_normal(yp.data_ptr(), M * D, seed, step.data_ptr(), _st(bk.dev))
  sh_e, dz_e = mmd_shard_run(bk, ws, xt, yp, kernel, W, M, cf, cg, 0, seed=seed, step=step)
  sh_p, dz_p = mmd_shard_run(bk, ws, xt, None, kernel, W, M, cf, cg, 0, seed=seed, step=step)
  for r in range(W):
    assert torch.equal(dz_p[r], dz_e[r]), r
  ref_p = np_mmd(x, yp.cpu().numpy(), kernel)
  assert_value(total(sh_e) / coef, ref_p)
  assert_value(total(sh_p) / coef, ref_p)
  assert_grad(torch.cat(dz_p).cpu().numpy() / cgrad, np_mmd_grad(x, yp.cpu().numpy(), kernel))


# ---- DIP ------------------------------------------------------------------------------------------------------------
def dip_inputs(bk, case):
  """(p [N, 2D], W, lambda_diag, lambda_offdiag, coef_grad)"""
  kind, D, type2 = case
  if kind == 'far':   # the far=True inputs of test_dip_kernel_matches_float64: means far from zero
    N = 96 if bk.name == 'sim' else 512
    rng = np.random.default_rng(D * 7 + type2)
    p = np.concatenate([rng.standard_normal((N, D)) * 1.3 + 0.2 + 1e3, rng.standard_normal((N, D)) * 0.5 - 0.5], 1)
    return p.astype(np.float32), 4, 1.5, 2.5, 0.75
  N, W = (64, 4) if kind == 'w4' else (8, 8)   # (8, 8): B_local = 1, blocks of n = 1 and a zero M2
  rng = np.random.default_rng(9)   # the inputs of test_dip_moments_finish_equal_fused
  p = np.concatenate([rng.standard_normal((N, D)) + 3.0, rng.standard_normal((N, D))], 1)
  return p.astype(np.float32), W, 1.0, 2.0, None


DIP_CASES = [('w4', 5), ('w8_bl1', 5), ('far', 1), ('far', 4), ('far', 10), ('far', 45)]


@pytest.mark.parametrize('type2', [0, 1])
@pytest.mark.parametrize('kind,D', DIP_CASES)
def test_dip_moments_finish_shards(bk, kind, D, type2):
  L = bk.L
  p, W, ld, lo, cgrad = dip_inputs(bk, (kind, D, type2))
  N, Bl, bs = p.shape[0], p.shape[0] // W, 1 + 2 * D + D * D
  pt = bk.T(p)
  cg = bk.T(np.array([cgrad], np.float32)) if cgrad is not None else None
  blocks = bk.zeros(W * bs)   # (the all-gather, rank order)
  for r in range(W):
    L.odin_dip_moments(pt[r * Bl:].data_ptr(), blocks[r * bs:].data_ptr(), Bl, D, _st(bk.dev))
  val, rdl, rds = np_dip(p, not type2, lo=lo, ld=ld)
  values = []
  for r in range(W):
    ws = bk.zeros(L.odin_dip_workspace(W, D))
    dl, ds = bk.full((Bl, D), float('nan')), bk.full((Bl, D), float('nan'))
    L.odin_dip_finish(blocks.data_ptr(), W, pt[r * Bl:].data_ptr(), ws.data_ptr(), dl.data_ptr(), ds.data_ptr(), None,
                      cg.data_ptr() if cg is not None else None, Bl, D, type2, ld, lo, _st(bk.dev))
    assert_value(float(ws[0]), val)
    assert_grad(dl.cpu().numpy() / (cgrad or 1.0), rdl[r * Bl:(r + 1) * Bl])
    if type2:
      assert_grad(ds.cpu().numpy() / (cgrad or 1.0), rds[r * Bl:(r + 1) * Bl])
    else:
      assert float(ds.abs().max()) == 0.0
    values.append(ws[:1].clone())
  for r in range(1, W):   # the whole batch's value: the same on every rank
    assert torch.equal(values[r], values[0]), r


# ---- random permutations --------------------------------------------------------------------------------------------
@pytest.mark.parametrize('D', [1, 10])
@pytest.mark.parametrize('B', [1, 63, 256, 257, 1000])   # 256 threads stride over B: up to four trips of the loop
def test_random_perm_sizes(bk, B, D):
  """the portable properties of test_permute_and_dtc_and_rng (B = 128 there) on both sides of the 256-thread stride"""
  L = bk.L
  z = np.random.default_rng(B + D).standard_normal((B, D)).astype(np.float32)
  tz = bk.T(z)
  step, step2 = bk.T([3], torch.int32), bk.T([4], torch.int32)

  def perm_of(s):
    perm = bk.full((B, D), -1.0).to(torch.int32)
    L.odin_random_perm(perm.data_ptr(), B, D, 1234, s.data_ptr(), _st(bk.dev))
    return perm
  perm = perm_of(step)
  pn = perm.cpu().numpy()
  for l in range(D):
    assert np.array_equal(np.sort(pn[:, l]), np.arange(B)), l
  out = bk.full((B, D), float('nan'))
  L.odin_permute_dims(tz.data_ptr(), perm.data_ptr(), out.data_ptr(), B, D, _st(bk.dev))
  assert np.array_equal(out.cpu().numpy(), vo.permute_dims(z, pn.astype(np.int64)))   # (a gather: exact)
  # the two as one launch: the same permutation, the same rows
  perm2, out2 = bk.full((B, D), -1.0).to(torch.int32), bk.full((B, D), float('nan'))
  L.odin_random_permute_dims(perm2.data_ptr(), tz.data_ptr(), out2.data_ptr(), B, D, 1234, step.data_ptr(), _st(bk.dev))
  assert torch.equal(perm2, perm) and torch.equal(out2, out)
  # deterministic in (seed, step); another step draws another permutation (B = 1 has only one)
  assert torch.equal(perm_of(step), perm)
  if B > 1:
    assert not torch.equal(perm_of(step2), perm)
