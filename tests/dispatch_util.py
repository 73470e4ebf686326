"""Which kernel family serves which layer: the table behind tests/test_dispatch_table.py and, run as a script, its
recorder (``python -m tests.dispatch_util sim|hip`` merges one backend's answers into tests/golden/dispatch_table.json).

A case is one conv / deconv / dense layer.  Recorded without a launch: the row counts of every dry run and the answers
of the ``*_keeps_range`` / ``*_reads_x_range`` predicates (key ``sim`` / ``hip``: the rows depend on odin_num_cus()).
Recorded with one launch per op on zero-filled buffers: odin_debug_last_path() (key ``hip_paths`` for every case; key
``sim_paths`` for SIM_PATH_CASES, the smallest shape of a family each, with the flop thresholds zeroed).

The record pins what the dispatch did BEFORE a change to it: run the recorder on the parent commit of such a change (this
file copied into that checkout) and commit its output unedited.  Recording on the changed tree makes the tests vacuous."""
import ctypes as C
import json
import os
import sys

import torch

from odin_ai_amd import _lib
from odin_ai_amd.engine import ParamLayout, build_layers
from odin_ai_amd.networks import get_networks
from oracle import vae_oracle as vo

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'dispatch_table.json')


def _speech():
  nets = get_networks('speech', n_frames=96, n_mels=80)
  return nets['encoder'].layers, nets['decoder'].layers, nets['encoder'].input_shape, nets['latents'].event_shape[0]


# the networks behind the benchmark's workloads at their batch sizes (tests/test_gpu_parity.py: FULL); C1 = maps of
# the 1x1 head behind the fused Bernoulli tail
NETS = [
    ('dsprites_b256', lambda: vo.dsprites_spec(1), 256),
    ('shapes3d_b128', lambda: vo.dsprites_spec(3), 128),
    ('celeba_b512', lambda: vo.celeba_spec(45, 3), 512),
    ('mnist_conv_b128', lambda: vo.mnist_conv_spec(), 128),
    ('mnist_dense_b128', lambda: vo.mnist_dense_spec(), 128),
    ('speech_b256', _speech, 256),
]


def conv_case(kind, B, H, W, Cin, Cout, K, S, act='elu', aux_act='elu', center=False, **opt):
  """a Conv2D (SAME pads on the input) or Conv2DTranspose (SAME pads on the output) layer"""
  if kind == 'conv':
    OH, pt, _ = vo.same_pads(H, K, S)
    OW, pl, _ = vo.same_pads(W, K, S)
  else:
    OH, OW = H * S, W * S
    pt, pl = vo.same_pads(OH, K, S)[1], vo.same_pads(OW, K, S)[1]
  return dict(kind=kind, B=B, H=H, W=W, Cin=Cin, OH=OH, OW=OW, Cout=Cout, K=K, S=S, pt=pt, pl=pl, act=act,
              aux_act=aux_act, center=bool(center), **opt)


def dense_case(B, K, N, act='linear', aux_act='linear', **opt):
  return dict(kind='dense', B=B, K=K, N=N, act=act, aux_act=aux_act, **opt)


def _net_cases():
  out = {}
  for name, spec, B in NETS:
    enc, dec, in_shape, zdim = spec()
    recs_e, flat = build_layers('enc', enc, tuple(in_shape), ParamLayout())
    recs_d, _ = build_layers('dec', dec, (zdim,), ParamLayout())
    prev = 'linear'
    layers = [('enc%d' % i, r) for i, r in enumerate(recs_e)] + [('latent', None)] + \
             [('dec%d' % i, r) for i, r in enumerate(recs_d)]
    for lname, r in layers:
      if r is None:   # the projection onto the posterior's parameters
        c = dense_case(B, int(flat[0]), 2 * zdim, 'linear', prev)
        prev = 'linear'
      elif r.kind == 'dense':
        c = dense_case(B, r.K, r.N, r.act, prev)
        prev = r.act
      else:
        d = r.desc
        c = dict(kind=r.kind, B=B, H=d['H'], W=d['W'], Cin=d['Cin'], OH=d['OH'], OW=d['OW'], Cout=d['Cout'], K=d['K'],
                 S=d['stride'], pt=d['pad_t'], pl=d['pad_l'], act=r.act, aux_act=prev, center=bool(r.center))
        prev = r.act
      out['%s/%s' % (name, lname)] = c
  # FactorVAE's discriminator: 5 x 1000 units (leaky layers run as linear + pointwise) over 10 latents, 2 logits
  for i, (K, N) in enumerate([(10, 1000), (1000, 1000), (1000, 2)]):
    out['disc1000_b256/d%d' % i] = dense_case(256, K, N)
  return out


def _edge_cases():
  e = {}
  # column-sum slab and more than ODIN_MAX_COLSUM_BLOCKS implicit-GEMM tiles: the slab sends the layer elsewhere
  # (fp32 implicit GEMM: below 1.2 GFLOP; 72 x 16 x 16 pixels = 576 tiles)
  e['slab_conv_dgrad_many_tiles'] = conv_case('conv', 72, 16, 16, 24, 8, 4, 2, slab=True)
  e['slab_deconv_dgrad_many_tiles'] = conv_case('deconv', 72, 16, 16, 24, 8, 4, 2, slab=True)
  e['slab_conv_dgrad_few_tiles'] = conv_case('conv', 64, 8, 8, 64, 64, 4, 2, slab=True)
  e['slab_deconv_dgrad_few_tiles'] = conv_case('deconv', 64, 4, 4, 64, 64, 4, 2, slab=True)
  e['slab_smalldeconv'] = conv_case('deconv', 256, 4, 4, 8, 64, 4, 2, aux_act='linear', slab=True)
  e['nobias_conv_k4s2'] = conv_case('conv', 256, 32, 32, 32, 32, 4, 2, bias=False)
  e['nobias_conv_k5s1'] = conv_case('conv', 128, 28, 28, 32, 32, 5, 1, bias=False)
  e['nobias_deconv_k4s2'] = conv_case('deconv', 256, 16, 16, 32, 32, 4, 2, bias=False)
  e['nobias_smalldeconv'] = conv_case('deconv', 256, 4, 4, 8, 64, 4, 2, bias=False)
  e['nobias_deconv_thin'] = conv_case('deconv', 128, 7, 7, 4, 64, 5, 2, bias=False)
  e['elu_noaux_conv_k4s2'] = conv_case('conv', 256, 32, 32, 32, 32, 4, 2, aux=False)
  e['elu_noaux_conv_c64'] = conv_case('conv', 256, 16, 16, 32, 64, 4, 2, aux=False)
  e['elu_noaux_deconv_k4s2'] = conv_case('deconv', 256, 16, 16, 32, 32, 4, 2, aux=False)
  e['elu_noaux_deconv_c64'] = conv_case('deconv', 256, 8, 8, 64, 64, 4, 2, aux=False)
  for ci in (1, 3, 4, 12):
    e['cin%d_conv_k4s2' % ci] = conv_case('conv', 64, 32, 32, ci, 32, 4, 2, aux_act='linear')
    e['cin%d_conv_k5s1' % ci] = conv_case('conv', 64, 28, 28, ci, 32, 5, 1, aux_act='linear')
    e['cin%d_conv_k1' % ci] = conv_case('conv', 64, 32, 32, 32, ci, 1, 1, act='linear')
    e['cin%d_deconv_k4s2' % ci] = conv_case('deconv', 64, 4, 4, ci, 64, 4, 2, aux_act='linear')
    e['cin%d_deconv_k5s2' % ci] = conv_case('deconv', 64, 7, 7, ci, 64, 5, 2, aux_act='linear')
  e['center_conv_k4s2_c1'] = conv_case('conv', 256, 64, 64, 1, 32, 4, 2, aux_act='linear', center=True)
  e['center_conv_k4s2_c32'] = conv_case('conv', 256, 32, 32, 32, 32, 4, 2, center=True)
  e['center_conv_k4s2_c64'] = conv_case('conv', 256, 8, 8, 64, 64, 4, 2, center=True)
  e['center_conv_k5s1'] = conv_case('conv', 128, 28, 28, 32, 32, 5, 1, center=True)
  e['center_deconv_k4s2'] = conv_case('deconv', 256, 16, 16, 32, 32, 4, 2, center=True)
  e['relu_conv_k4s2'] = conv_case('conv', 256, 32, 32, 32, 32, 4, 2, act='relu', aux_act='relu')
  e['relu_deconv_k4s2'] = conv_case('deconv', 256, 16, 16, 32, 32, 4, 2, act='relu', aux_act='relu')
  e['odd_conv_k3s1'] = conv_case('conv', 8, 9, 7, 5, 6, 3, 1)
  e['odd_deconv_k3s2'] = conv_case('deconv', 8, 5, 3, 6, 5, 3, 2)
  # one Dense shape per branch of the chains
  e['dense_tiny'] = dense_case(64, 10, 4)
  e['dense_thin_k'] = dense_case(256, 10, 1000)
  e['dense_thin_n'] = dense_case(256, 1000, 2)
  e['dense_thin_k_unaligned'] = dense_case(256, 10, 1000, unaligned=True)
  e['dense_thin_n_unaligned'] = dense_case(256, 1000, 2, unaligned=True)
  e['dense_h'] = dense_case(256, 1000, 1000, act='relu', aux_act='relu')
  e['dense_h_slab'] = dense_case(256, 512, 512, slab=True)
  e['dense_igemm'] = dense_case(128, 128, 64, act='relu')
  e['dense_igemm_slab'] = dense_case(256, 128, 64, slab=True)
  e['dense_gemm'] = dense_case(32, 100, 60)
  e['dense_gemm_odd'] = dense_case(16, 300, 20, act='elu', aux_act='elu')
  e['dense_generic'] = dense_case(5000, 100, 60)
  e['dense_wide_k'] = dense_case(3, 5000, 37)
  e['dense_bwd_no_wgrad'] = dense_case(256, 1000, 1000, want_wgrad=False)
  e['dense_bwd_no_dgrad'] = dense_case(256, 1000, 1000, want_dgrad=False)
  e['dense_igemm_bwd_no_wgrad'] = dense_case(128, 128, 64, want_wgrad=False)
  e['dense_igemm_bwd_no_dgrad'] = dense_case(128, 128, 64, want_dgrad=False)
  return e


def all_cases():
  c = _net_cases()
  c.update(_edge_cases())
  return c


# the simulator's launches: the smallest shape each family's predicate accepts (thresholds zeroed by the debug setters)
SIM_PATH_CASES = {
    'sim_pw1x1': conv_case('conv', 2, 4, 4, 8, 1, 1, 1, act='linear'),
    'sim_smallc': conv_case('conv', 2, 8, 8, 1, 32, 4, 2, aux_act='linear'),
    'sim_conv_k4s2_c32': conv_case('conv', 2, 16, 16, 32, 32, 4, 2),
    'sim_conv_k4s2_c64': conv_case('conv', 2, 8, 8, 32, 64, 4, 2),
    'sim_conv_k5s1': conv_case('conv', 1, 8, 8, 32, 32, 5, 1),
    'sim_conv_generic': conv_case('conv', 1, 5, 5, 3, 5, 3, 1),
    'sim_smalldeconv': conv_case('deconv', 2, 4, 4, 8, 64, 4, 2, aux_act='linear'),
    'sim_deconv_k4s2_c32': conv_case('deconv', 2, 8, 8, 32, 32, 4, 2),
    'sim_deconv_k4s2_c64': conv_case('deconv', 2, 4, 4, 64, 64, 4, 2),
    'sim_deconv_generic': conv_case('deconv', 1, 3, 3, 3, 5, 3, 2),
    'sim_dense_tiny': dense_case(4, 10, 4),
    'sim_dense_igemm': dense_case(16, 128, 64),
}


def _desc(c):
  return _lib.conv_desc(c['B'], c['H'], c['W'], c['Cin'], c['OH'], c['OW'], c['Cout'], c['K'], c['S'], c['pt'], c['pl'],
                        c['act'], c['center'])


def _ptr(t):
  return None if t is None else t.data_ptr()


def record_static(L, c):
  """dry-run row counts and predicate answers of one case: nothing is launched"""
  r = {}
  rows, rows2 = C.c_int(-1), C.c_int(-1)
  slab = torch.zeros(4)   # (a dry run tests the pointer only)

  def dry(fn, *a):
    rows.value = rows2.value = -1
    try:
      fn(*a)
    except _lib.OdinError as e:
      return 'error: ' + str(e).split(':', 1)[-1].strip()
    return None

  aux_act = _lib.ACT[c['aux_act']]
  if c['kind'] == 'dense':
    B, K, N = c['B'], c['K'], c['N']
    r['wgrad_rows'] = dry(L.odin_dense_wgrad, None, None, None, C.byref(rows), B, K, N, None) or rows.value
    for key, s in (('dgrad_rows', None), ('dgrad_rows_slab', slab.data_ptr())):
      r[key] = dry(L.odin_dense_dgrad, None, None, None, aux_act, None, s, C.byref(rows), B, K, N, None) or rows.value
    for key, s in (('bwd_rows', None), ('bwd_rows_slab', slab.data_ptr())):
      r[key] = dry(L.odin_dense_bwd, None, None, None, None, aux_act, None, s, C.byref(rows), None, C.byref(rows2),
                   B, K, N, int(c.get('want_wgrad', True)), int(c.get('want_dgrad', True)), None, None, None) or \
          [rows.value, rows2.value]
    r['dgrad_keeps_range'] = L.odin_dense_dgrad_keeps_range(B, K, N)
    r['reads_x_range'] = L.odin_dense_reads_x_range(B, K, N)
    return r
  d = _desc(c)
  op = 'odin_%s2d_' % c['kind']
  r['wgrad_rows'] = dry(getattr(L, op + 'wgrad'), None, None, None, C.byref(rows), C.byref(d), None) or rows.value
  for key, s in (('dgrad_rows', None), ('dgrad_rows_slab', slab.data_ptr())):
    r[key] = dry(getattr(L, op + 'dgrad'), None, None, None, aux_act, None, s, C.byref(rows), C.byref(d), None) or \
        rows.value
  for key, s in (('bwd_rows', None), ('bwd_rows_slab', slab.data_ptr())):
    r[key] = dry(getattr(L, op + 'bwd'), None, None, None, None, aux_act, None, s, C.byref(rows), None, C.byref(rows2),
                 C.byref(d), None) or [rows.value, rows2.value]
  for c1 in (1, 3):
    r['tail_rows_c%d' % c1] = dry(L.odin_bernoulli_tail_fwd_bwd, int(c['kind'] == 'deconv'), None, None, None, None, None,
                                  None, None, None, None, C.byref(rows2), None, C.byref(rows), None, C.byref(d), c1,
                                  None) or [rows.value, rows2.value]
    r['tail_keeps_range_c%d' % c1] = L.odin_bernoulli_tail_keeps_range(int(c['kind'] == 'deconv'), C.byref(d), c1)
  for a in ('linear', 'elu', 'relu'):
    r['dgrad_keeps_range_' + a] = getattr(L, op + 'dgrad_keeps_range')(C.byref(d), _lib.ACT[a])
  r['reads_x_range'] = getattr(L, op + 'reads_x_range')(C.byref(d))
  return r


def record_paths(L, dev, c):
  """odin_debug_last_path() after each op of one case, launched on zero-filled buffers"""
  r = {}
  rows, rows2 = C.c_int(0), C.c_int(0)
  max_rows = L.odin_max_slab_rows()
  st = None
  if torch.device(dev).type == 'cuda':
    st = torch.cuda.current_stream().cuda_stream

  def Z(n, words=False):
    return torch.zeros(int(n), dtype=torch.int32 if words else torch.float32, device=dev)

  def path(fn, *a):
    try:
      fn(*a)
    except _lib.OdinError as e:
      return 'error: ' + str(e).split(':', 1)[-1].strip()
    if torch.device(dev).type == 'cuda':
      torch.cuda.synchronize()
    return L.odin_debug_last_path().decode()

  aux_act = _lib.ACT[c['aux_act']]
  has_aux = c.get('aux', True) and aux_act != 0
  if c['kind'] == 'dense':
    B, K, N = c['B'], c['K'], c['N']
    off = 1 if c.get('unaligned') else 0   # (4 bytes past a 16-byte boundary)
    x, w, b, y = Z(B * K + 4)[off:], Z(K * N + 4)[off:], Z(N + 4)[off:], Z(B * N + 4)[off:]
    dx, aux = Z(B * K + 4)[off:], (Z(B * K + 4)[off:] if has_aux else None)
    L.odin_dense_wgrad(None, None, None, C.byref(rows), B, K, N, None)
    wslab = Z((max(rows.value, 1) + 1) * (K * N + N) + 4)[off:]
    colsum = Z(max_rows * K) if c.get('slab') else None
    r['fwd'] = path(L.odin_dense_fwd, _ptr(x), _ptr(w), _ptr(b), _ptr(y), B, K, N, _lib.ACT[c['act']], st)
    r['wgrad'] = path(L.odin_dense_wgrad, _ptr(x), _ptr(y), _ptr(wslab), C.byref(rows), B, K, N, st)
    r['dgrad'] = path(L.odin_dense_dgrad, _ptr(y), _ptr(w), _ptr(aux), aux_act, _ptr(dx), None, C.byref(rows), B, K, N,
                      st)
    if colsum is not None:
      r['dgrad_slab'] = path(L.odin_dense_dgrad, _ptr(y), _ptr(w), _ptr(aux), aux_act, _ptr(dx), _ptr(colsum),
                             C.byref(rows), B, K, N, st)
    r['bwd'] = path(L.odin_dense_bwd, _ptr(x), _ptr(y), _ptr(w), _ptr(aux), aux_act, _ptr(dx), _ptr(colsum),
                    C.byref(rows), _ptr(wslab), C.byref(rows2), B, K, N, int(c.get('want_wgrad', True)),
                    int(c.get('want_dgrad', True)), None, None, st)
    return r
  d = _desc(c)
  B, Ci, Co, K = c['B'], c['Cin'], c['Cout'], c['K']
  nx, ny = B * c['H'] * c['W'] * Ci, B * c['OH'] * c['OW'] * Co
  op = 'odin_%s2d_' % c['kind']
  x, y, dx = Z(nx), Z(ny), Z(nx)
  w, b = Z(K * K * Ci * Co), (Z(Co) if c.get('bias', True) else None)
  aux = Z(nx) if has_aux else None
  stride = K * K * Ci * Co + Co
  getattr(L, op + 'bwd')(None, None, None, None, aux_act, None, None, C.byref(rows), None, C.byref(rows2), C.byref(d), None)
  n_w = rows2.value
  getattr(L, op + 'wgrad')(None, None, None, C.byref(rows2), C.byref(d), None)
  wslab = Z((max(n_w, rows2.value, 1) + 1) * stride)
  colsum = Z(max_rows * Ci) if c.get('slab') else None
  r['fwd'] = path(getattr(L, op + 'fwd'), _ptr(x), _ptr(w), _ptr(b), _ptr(y), C.byref(d), st)
  r['wgrad'] = path(getattr(L, op + 'wgrad'), _ptr(x), _ptr(y), _ptr(wslab), C.byref(rows), C.byref(d), st)
  r['dgrad'] = path(getattr(L, op + 'dgrad'), _ptr(y), _ptr(w), _ptr(aux), aux_act, _ptr(dx), None, C.byref(rows),
                    C.byref(d), st)
  if colsum is not None:
    r['dgrad_slab'] = path(getattr(L, op + 'dgrad'), _ptr(y), _ptr(w), _ptr(aux), aux_act, _ptr(dx), _ptr(colsum),
                           C.byref(rows), C.byref(d), st)
  r['bwd'] = path(getattr(L, op + 'bwd'), _ptr(x), _ptr(y), _ptr(w), _ptr(aux), aux_act, _ptr(dx), _ptr(colsum),
                  C.byref(rows), _ptr(wslab), C.byref(rows2), C.byref(d), st)
  # the fused Bernoulli tail where the engine would plan it: at most 32 maps, an image of more than one tile
  if Co <= 32 and c['OH'] * c['OW'] > 128 and b is not None and Ci % 4 == 0:
    for c1 in (1, 3):
      try:
        L.odin_bernoulli_tail_fwd_bwd(int(c['kind'] == 'deconv'), None, None, None, None, None, None, None, None, None,
                                      C.byref(rows2), None, C.byref(rows), None, C.byref(d), c1, None)
      except _lib.OdinError as e:
        r['tail_c%d' % c1] = 'error: ' + str(e).split(':', 1)[-1].strip()
        continue
      npix = B * c['OH'] * c['OW']
      w1, b1, tgt, logits, scale = Z(Co * c1), Z(c1), Z(npix * c1), Z(npix * c1), Z(4)
      part, tslab = Z(B * max(rows2.value, 1)), Z(max(rows.value, 1) * (Co * c1 + c1 + Co))
      r['tail_c%d' % c1] = path(L.odin_bernoulli_tail_fwd_bwd, int(c['kind'] == 'deconv'), _ptr(x), _ptr(w), _ptr(b),
                                _ptr(w1), _ptr(b1), _ptr(tgt), _ptr(logits), _ptr(y), _ptr(part), C.byref(rows2),
                                _ptr(tslab), C.byref(rows), _ptr(scale), C.byref(d), c1, st)
  return r


def record(L, dev, backend):
  """-> {key: {case: answers}} of one backend ('sim' or 'hip'), the whole table once more under ODIN_EXACT_FP32"""
  out = {}
  for exact in (False, True):
    sfx = '_exact_fp32' if exact else ''
    if exact:
      os.environ['ODIN_EXACT_FP32'] = '1'
      os.putenv('ODIN_EXACT_FP32', '1')
    try:
      out[backend + sfx] = {n: record_static(L, c) for n, c in all_cases().items()}
      if backend == 'hip':
        out['hip_paths' + sfx] = {n: record_paths(L, dev, c) for n, c in all_cases().items()}
      else:
        old = L.odin_debug_blk_min_flop(0.0), L.odin_debug_igemm_h_min_flop(0.0)
        try:
          out['sim_paths' + sfx] = {n: record_paths(L, dev, c) for n, c in SIM_PATH_CASES.items()}
        finally:
          L.odin_debug_blk_min_flop(old[0])
          L.odin_debug_igemm_h_min_flop(old[1])
    finally:
      if exact:
        os.environ.pop('ODIN_EXACT_FP32', None)
        os.unsetenv('ODIN_EXACT_FP32')
  return out


def main(argv):
  backend = argv[1] if len(argv) > 1 else 'sim'
  dst = argv[2] if len(argv) > 2 else GOLDEN
  if backend == 'sim':
    from tests.simutil import sim_lib
    got = record(sim_lib(), 'cpu', 'sim')
  else:
    got = record(_lib.load(), 'cuda:0', 'hip')
  table = {}
  if os.path.exists(dst):
    with open(dst) as f:
      table = json.load(f)
  table.update(got)
  with open(dst, 'w') as f:
    json.dump(table, f, indent=0, sort_keys=True)
    f.write('\n')


if __name__ == '__main__':
  main(sys.argv)
