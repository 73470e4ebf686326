"""odin_decoder_tail_chain: decoder3's forward inside the fused Bernoulli tail's launch (tconv_planes.hip:
tconv_chain2_kernel) against the two separate calls and against float64, and the engine option that uses it.

What is compared how:
  * y3, the logits, dL/dy (g_out) and the two range words do not depend on how the images are dealt to workgroups:
    equal to the separate calls bit for bit at every batch size.
  * the per-sample log-likelihood and the reduced slab are sums whose ORDER follows the partition (a workgroup's lanes
    accumulate over all its tiles): within 1e-6 of their maximum of the separate calls' at the small batches, where the
    chain gives a workgroup a whole image and the tail alone gives it one tile; bit-identical -- the raw slab rows and
    the per-tile partials included -- where the dry run reports the same partition (test_bit_identity_*).
  * everything within 1e-4 of its maximum of float64 (the tolerance of tests/test_ops.py).
"""
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from odin_ai_amd import _lib
from odin_ai_amd.engine import VAEEngine
from oracle import vae_oracle as vo
from tests.engine_util import Recorder
from tests.parity_util import reduce_slab

CO = 32   # channels of decoder3's and decoder4's outputs


def draw(B, C1, seed=3, x_scale=None, zero_b3=False):
  """the layers' real geometry: x [B, 16, 16, 64] -> y3 [B, 32, 32, 32] -> 64 x 64 x 32 -> C1 logit maps"""
  rng = np.random.default_rng(seed)
  d = dict(x=rng.standard_normal((B, 16, 16, 64)), w3=rng.standard_normal((4, 4, CO, 64)) * 0.1,
           b3=rng.standard_normal(CO) * 0.1, w4=rng.standard_normal((4, 4, CO, CO)) * 0.2, b4=rng.standard_normal(CO) * 0.1,
           w1=rng.standard_normal((1, 1, CO, C1)) * 0.3, b1=rng.standard_normal(C1) * 0.1,
           tgt=np.clip(rng.random((B, 64, 64, C1)), 1e-6, 1 - 1e-6))
  if zero_b3:
    d['b3'] = np.zeros(CO)
  if x_scale is not None:
    d['x'] = d['x'] * np.asarray(x_scale, np.float64).reshape(-1, 1, 1, 1)
  return {k: v.astype(np.float32) for k, v in d.items()}


def ref64(bk, d):
  """float64 on the fp32 values the kernels read (torch on the backend's device); NHWC results"""
  t = {k: bk.T(v).double() for k, v in d.items()}
  B = t['x'].shape[0]
  wt = lambda w: w.permute(3, 2, 0, 1)   # [kh, kw, Co, Ci] -> conv_transpose2d's [Ci, Co, kh, kw]
  y3 = F.elu(F.conv_transpose2d(t['x'].permute(0, 3, 1, 2), wt(t['w3']), t['b3'], stride=2, padding=1))
  y4 = F.elu(F.conv_transpose2d(y3, wt(t['w4']), t['b4'], stride=2, padding=1)).permute(0, 2, 3, 1)
  w1 = t['w1'][0, 0]
  lg = y4 @ w1 + t['b1']
  llk = (t['tgt'] * lg - F.softplus(lg)).sum((1, 2, 3))
  dl = (torch.sigmoid(lg) - t['tgt']) / B
  g = (dl @ w1.T) * (1.0 + torch.clamp(y4, max=0.0))
  red = torch.cat([torch.einsum('bhwc,bhwo->co', y4, dl).reshape(-1), dl.sum((0, 1, 2)), g.sum((0, 1, 2))])
  return dict(y3=y3.permute(0, 2, 3, 1), logits=lg, g=g, llk=llk, red=red)


def descs(B):
  d3 = _lib.conv_desc(B, 16, 16, 64, 32, 32, CO, 4, 2, 1, 1, 'elu')
  d4 = _lib.conv_desc(B, 32, 32, CO, 64, 64, CO, 4, 2, 1, 1, 'elu')
  return d3, d4


def run(bk, d, chain):
  """the chain, or odin_deconv2d_fwd + odin_bernoulli_tail_fwd_bwd, on device tensors of `d` -> every output"""
  L = bk.L
  t = {k: bk.T(v) for k, v in d.items()}
  B, C1 = d['x'].shape[0], d['tgt'].shape[-1]
  d3, d4 = descs(B)
  xw, yw, dyw = (bk.zeros(2048, dtype=torch.int32) for _ in range(3))
  L.odin_absmax(t['x'].data_ptr(), t['x'].numel(), xw.data_ptr(), None)
  d3.x_amax, d3.y_amax, d4.x_amax, d4.dy_amax = xw.data_ptr(), yw.data_ptr(), yw.data_ptr(), dyw.data_ptr()
  sc = bk.T([1.0 / B])
  rows, npart, same = C.c_int(0), C.c_int(0), C.c_int(-1)
  if chain:
    dry = lambda: L.odin_decoder_tail_chain(None, None, None, None, C.byref(d3), None, None, None, None, None, None, None,
                                            None, C.byref(npart), None, C.byref(rows), C.byref(same), None, C.byref(d4),
                                            C1, None)
  else:
    dry = lambda: L.odin_bernoulli_tail_fwd_bwd(1, None, None, None, None, None, None, None, None, None, C.byref(npart),
                                                None, C.byref(rows), None, C.byref(d4), C1, None)
  dry()
  n = CO * C1 + C1 + CO
  o = dict(y3=bk.full((B, 32, 32, CO), float('nan')), logits=bk.full((B, 64, 64, C1), float('nan')),
           g=bk.full((B, 64, 64, CO), float('nan')), part=bk.full((B * npart.value,), float('nan')),
           slab=bk.full((rows.value, n), float('nan')))
  p = lambda k: (t[k] if k in t else o[k]).data_ptr()
  if chain:
    L.odin_decoder_tail_chain(p('x'), p('w3'), p('b3'), p('y3'), C.byref(d3), p('w4'), p('b4'), p('w1'), p('b1'), p('tgt'),
                              p('logits'), p('g'), p('part'), C.byref(npart), p('slab'), C.byref(rows), C.byref(same),
                              sc.data_ptr(), C.byref(d4), C1, None)
    path = L.odin_debug_last_path().decode()
    assert path == 'tconv_chain2(f16x2)', path
  else:
    L.odin_deconv2d_fwd(p('x'), p('w3'), p('b3'), p('y3'), C.byref(d3), None)
    assert 'tconv_planes' in L.odin_debug_last_path().decode()
    L.odin_bernoulli_tail_fwd_bwd(1, p('y3'), p('w4'), p('b4'), p('w1'), p('b1'), p('tgt'), p('logits'), p('g'), p('part'),
                                  C.byref(npart), p('slab'), C.byref(rows), sc.data_ptr(), C.byref(d4), C1, None)
    assert 'tconv_planes' in L.odin_debug_last_path().decode()
  # (a range word is 32 sub-words, one per workgroup slot: the bound is their maximum -- which workgroup commits to which
  # slot follows the grid, the bound does not)
  bound = lambda w: w.view(torch.float32).max().reshape(1)
  o.update(yw=bound(yw), dyw=bound(dyw), llk=o['part'].reshape(B, -1).sum(1), red=torch.tensor(reduce_slab(bk, o['slab'], rows.value, n)),
           same=same.value, rows=rows.value)
  return o


def rel(a, b):
  a, b = (np.asarray(v.cpu() if torch.is_tensor(v) else v, np.float64) for v in (a, b))
  return float(np.abs(a - b).max() / np.abs(b).max())


EXACT = ('y3', 'logits', 'g', 'yw', 'dyw')   # what does not depend on the partition
ALL = EXACT + ('part', 'slab')


def compare(bk, d, tag, again=False):
  sep, ch = run(bk, d, False), run(bk, d, True)
  ref = ref64(bk, d)
  for k in EXACT:
    assert torch.equal(ch[k], sep[k]), (tag, k)
  assert float(ch['yw']) == float(ch['y3'].abs().max())
  assert float(ch['dyw']) == float(ch['g'].abs().max())
  figs = {k: (rel(ch[k], sep[k]), rel(ch[k], ref[k])) for k in ('llk', 'red')}
  figs.update({k: (0.0, rel(ch[k], ref[k])) for k in ('y3', 'logits', 'g')})
  print(tag, 'rows', ch['rows'], 'same partition', ch['same'], {k: ('%.2e' % a, '%.2e' % b) for k, (a, b) in figs.items()})
  for k, (vs_sep, vs_ref) in figs.items():
    assert vs_sep <= 1e-6 and vs_ref <= 1e-4, (tag, k, vs_sep, vs_ref)
  if again:   # two runs are bit-identical
    ch2 = run(bk, d, True)
    for k in ALL:
      assert torch.equal(ch[k], ch2[k]), (tag, 'second run', k)
  return sep, ch


def _cus(bk):
  return torch.cuda.get_device_properties(0).multi_processor_count if bk.name == 'hip' else 16


def _check_rows(bk, B, rows):
  ipw = -(-B // min(_cus(bk), 512))   # whole images per workgroup, the chip filled once
  assert rows == -(-B // ipw)


@pytest.mark.parametrize('C1', [1, 3])
@pytest.mark.parametrize('B', [1, 3, 5])
def test_tail_chain_against_separate_calls_and_float64(bk, B, C1):
  """B = 1 (a single image), 3 and 5 (odd batches, fewer workgroups than CUs)"""
  # (the second run at B = 3, and at every batch on the GPU: a simulated image takes seconds)
  sep, ch = compare(bk, draw(B, C1), 'B=%d C1=%d' % (B, C1), again=B == 3 or bk.name == 'hip')
  _check_rows(bk, B, ch['rows'])


@pytest.mark.gpu
@pytest.mark.parametrize('C1', [1, 3])
def test_tail_chain_two_images_per_workgroup(C1):
  """B = CUs + 2: two images in every workgroup but a ragged last one (the simulator's 16 CUs would need B = 18 and
  minutes for the same shape of partition: GPU only)"""
  from tests.conftest import Backend
  bk = Backend('hip', _lib.load(), 'cuda:0')
  B = _cus(bk) + 2
  sep, ch = compare(bk, draw(B, C1), 'B=%d C1=%d' % (B, C1), again=True)
  _check_rows(bk, B, ch['rows'])
  assert ch['rows'] < B


@pytest.mark.gpu
@pytest.mark.parametrize('C1', [1, 3])
def test_bit_identity_where_the_partitions_coincide(C1):
  """B = 256: the dry run must report the stand-alone tail's partition (it does on any chip whose CU count divides 256
  images into whole images per workgroup the way the tail's tile count does -- an assertion, not a skip), and then every
  output, the raw slab rows and the per-tile partials included, equals the separate launches'"""
  from tests.conftest import Backend
  bk = Backend('hip', _lib.load(), 'cuda:0')
  d = draw(256, C1, seed=11)
  sep, ch = run(bk, d, False), run(bk, d, True)
  assert ch['same'] == 1 and ch['rows'] == sep['rows']
  for k in ALL:
    assert torch.equal(ch[k], sep[k]), k
  assert bool(torch.isfinite(ch['slab']).all()) and float(ch['slab'].abs().max()) > 0


def test_local_range_word(bk):
  """The tail scales y3 by the bound of its OWN workgroup's images, not by the batch's (the global word is incomplete
  while other workgroups are still in decoder3).  Image 1 of 3 is scaled by 1e-5 (no bias in decoder3, so that y3 scales
  with it): its bound falls below 2^-8 while the batch's stays inside the window; then the whole batch times 1e5: every
  bound beyond what an f16 plane holds.  1e-4 of the maximum against float64 either way, as
  test_plane_kernels_beyond_f16_range asks of the stand-alone kernels.  (In the second case decoder4's weights are drawn
  1e5 times smaller, so that y3 of order 1e5 meets logits of order 1: with logits of order 1e6 the sigmoid's gradient
  near a zero crossing is lost to the fp32 rounding of the logit itself -- 1e6 x 2^-24 = 0.06 absolute -- in ANY fp32
  evaluation, and the case would measure that instead of the planes.)"""
  for tag, s in (('one small image', [1.0, 1e-5, 1.0]), ('times 1e5', [1e5, 1.0, 1e5])):
    d = draw(3, 1, seed=5, x_scale=s, zero_b3=True)
    if tag == 'times 1e5':
      d['w4'] = (d['w4'] * 1e-5).astype(np.float32)
    ch, ref = run(bk, d, True), ref64(bk, d)
    y3max = ref['y3'].abs().amax((1, 2, 3)).tolist()
    if tag == 'one small image':
      assert y3max[1] < 2.0 ** -8 <= min(y3max[0], y3max[2]) and max(y3max) < 2.0 ** 15, y3max
    else:
      assert max(y3max) > 65504.0, y3max
    figs = {k: rel(ch[k], ref[k]) for k in ('y3', 'logits', 'g', 'llk', 'red')}
    print(tag, {k: '%.2e' % v for k, v in figs.items()})
    for k, v in figs.items():
      assert v <= 1e-4, (tag, k, v)
    assert float(ch['yw']) == float(ch['y3'].abs().max())


def test_switches_turn_the_chain_off(bk, monkeypatch):
  """ODIN_EXACT_FP32 sends both layers away from the plane kernels: the chain declines (-2)"""
  d3, d4 = descs(2)
  monkeypatch.setenv('ODIN_EXACT_FP32', '1')
  with pytest.raises(_lib.OdinError, match='rc=-2'):
    bk.L.odin_decoder_tail_chain(None, None, None, None, C.byref(d3), None, None, None, None, None, None, None, None, None,
                                 None, None, None, None, C.byref(d4), 1, None)
  monkeypatch.delenv('ODIN_EXACT_FP32')
  d3b = _lib.conv_desc(2, 8, 8, 64, 16, 16, CO, 4, 2, 1, 1, 'elu')   # (another geometry)
  with pytest.raises(_lib.OdinError, match='rc=-2'):
    bk.L.odin_decoder_tail_chain(None, None, None, None, C.byref(d3b), None, None, None, None, None, None, None, None, None,
                                 None, None, None, None, C.byref(d4), 1, None)


# ---- the engine ------------------------------------------------------------------------------------------------------

class _Rec(Recorder):
  """the recorder of tests/engine_util.py; with `live` False a call is recorded and NOT made (which launches a forward
  pass issues is host logic: the simulator need not compute a whole dSprites batch to show it)"""
  live = True

  def __getattr__(self, name):
    call = Recorder.__getattr__(self, name)
    if not name.startswith('odin_'):
      return call

    def maybe(*a):
      if self.live:
        return call(*a)
      self.calls.append(name)
      return 0
    return maybe


def _engine(bk, B, calls=None, **kw):
  enc, dec, in_shape, zdim = vo.dsprites_spec(1)
  lib = bk.L if calls is None else _Rec(bk.L, calls)
  eng = VAEEngine(enc, dec, in_shape, zdim, B, bk.dev, lib=lib, **kw)
  g = torch.Generator().manual_seed(2)
  eng.params.copy_((torch.randn(eng.params.numel(), generator=g) * 0.05).to(bk.dev))
  return eng


def _batch(bk, B):
  rng = np.random.default_rng(4)
  return bk.T(np.clip(rng.random((B, 64, 64, 1)), 1e-6, 1 - 1e-6)), bk.T(rng.standard_normal((B, 10)))


def test_engine_uses_the_chain_only_where_the_partitions_coincide(bk):
  """The dSprites spec through the recorder.  A batch of one image per CU: the dry run reports the tail's own partition
  and the forward pass issues the chain in place of decoder3's forward + the tail; chain_fwd=False never names it and
  issues those two.  A batch of 4 (the tail alone would deal single tiles): the engine asks once and keeps the two
  launches; so does an engine under debug_check_ranges."""
  tail = ['odin_deconv2d_fwd', 'odin_bernoulli_tail_fwd_bwd']
  fwd = {}
  for B in (_cus(bk), 4):
    x, eps = _batch(bk, B)
    for on in (True, False):
      calls = []
      eng = _engine(bk, B, calls, chain_fwd=on)
      assert calls.count('odin_decoder_tail_chain') == (1 if on else 0) and eng.fused_tail   # (the dry run)
      assert eng.chain_tail == (on and B != 4)
      eng.step_count = 1
      eng.set_hyper(beta=2.0)
      eng.lib.live = bk.name == 'hip'
      del calls[:]
      eng.forward(x, eps)
      fwd[B, on] = list(calls)
      if eng.chain_tail:
        del calls[:]
        eng.debug_check_ranges = lambda e: None
        eng.forward(x, eps)
        fwd[B, 'audit'] = list(calls)
  B = _cus(bk)
  i = fwd[B, True].index('odin_decoder_tail_chain')
  assert fwd[B, True][:i] + tail + fwd[B, True][i + 1:] == fwd[B, False]
  assert 'odin_decoder_tail_chain' not in fwd[B, False] + fwd[B, 'audit']
  j = fwd[B, 'audit'].index('odin_bernoulli_tail_fwd_bwd')
  assert fwd[B, 'audit'][j - 1:] == fwd[B, False][i:]
  assert fwd[4, True] == fwd[4, False] and 'odin_decoder_tail_chain' not in fwd[4, True]


@pytest.mark.gpu
def test_gpu_step_is_bit_identical_and_the_graph_replays_it():
  """B = 256: one train_step with and without the chain leaves the same gradients, parameters and loss terms bit for
  bit, and the captured graph of the chained step replays the eager one"""
  from tests.conftest import Backend
  bk = Backend('hip', _lib.load(), 'cuda:0')
  x, eps = _batch(bk, 256)
  res = {}
  for key, kw, use_graph in (('chain', {}, False), ('separate', dict(chain_fwd=False), False), ('graph', {}, True)):
    eng = _engine(bk, 256, **kw)
    assert eng.chain_tail == (key != 'separate')
    out = eng.train_step(x, eps, lr=1e-3, beta=2.0, use_graph=use_graph).clone()
    torch.cuda.synchronize()
    res[key] = [eng.grads.clone(), eng.params.clone(), out, eng.dec.outs[-1].clone(), eng.tail_slab.clone()]
  for key in ('separate', 'graph'):
    for a, b in zip(res['chain'], res[key]):
      assert torch.equal(a, b), key
  assert bool(torch.isfinite(res['chain'][0]).all()) and float(res['chain'][0].abs().max()) > 0
