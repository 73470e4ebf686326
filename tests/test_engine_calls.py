"""The library calls of VAEEngine, construction included, against the record of tests/golden/engine_calls.json: names,
order and arguments (tests/engine_util.py: Recorder) of a table of tiny engines, on the simulator and on the GPU.  The
fixture was recorded on the simulator.  One field differed on the GPU when it was recorded, every call's trailing stream:
it is compared on the simulator only."""
import json
import os

import pytest
import torch

from odin_ai_amd import _lib
from odin_ai_amd._lib import OdinError
from odin_ai_amd.engine import VAEEngine
from tests.engine_util import Recorder, case_data, dense_spec, head_spec, neck_spec, tiny16_spec, tiny_spec

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'engine_calls.json')


DENSE1 = ([('flatten',), ('dense', 24, 'relu')], [('dense', 64, 'linear'), ('reshape', (8, 8, 1))], (8, 8, 1), 4)
VQ = dict(vq_codes=5, vq_code_size=8)
FLAGS = ('neck', 'lat_block', 'fused_tail', 'gauss_head', '_used_neck', '_bwd_neck')
# name: (spec, engine keywords, run, the FLAGS the case is meant to find set).  run: 'step' / 'step2' = one / two train_steps,
# 'unfused' = forward(fused=False) + backward(), 'parts' = run_encoder, run_decoder, observation_llk
CASES = {
    'tiny': (tiny_spec(), {}, 'step2', 'lat_block gauss_head'),
    'tiny_unfused': (tiny_spec(), {}, 'unfused', 'lat_block gauss_head'),
    'tiny16': (tiny16_spec(), {}, 'step', 'lat_block fused_tail'),
    'tiny16_defer': (tiny16_spec(), dict(defer_wgrad=True), 'step', 'lat_block fused_tail'),
    'neck128': (neck_spec(5, 128), {}, 'step', 'neck lat_block fused_tail _used_neck _bwd_neck'),
    'neck256': (neck_spec(5, 256), {}, 'step', 'neck lat_block fused_tail _used_neck'),
    'gaussian_softplus1': (head_spec(2), dict(observation='gaussian_softplus1'), 'step', 'lat_block gauss_head'),
    'qlogistic': (head_spec(2), dict(observation='qlogistic'), 'step', 'lat_block'),
    'mixqlogistic': (head_spec(30), dict(observation='mixqlogistic'), 'step', 'lat_block'),
    'dense': (dense_spec(), {}, 'step', 'lat_block'),
    'free_bits': (tiny_spec(), dict(analytic=True, free_bits=0.3), 'step', 'lat_block gauss_head'),
    'capacity': (tiny_spec(), dict(capacity=True), 'step', 'lat_block gauss_head'),
    'betatc': (tiny_spec(), dict(tc='betatc'), 'step', 'lat_block gauss_head'),
    'mmd': (tiny_spec(), dict(latent_reg='mmd', mmd_prior_samples=9), 'step', 'lat_block gauss_head'),
    'dip_i': (tiny_spec(), dict(latent_reg='dip_i'), 'step', 'lat_block gauss_head'),
    'dip_ii': (tiny_spec(), dict(latent_reg='dip_ii'), 'step', 'lat_block gauss_head'),
    'vamprior': (tiny_spec(), dict(vamprior_components=3), 'step', 'lat_block gauss_head'),
    'vq': (tiny_spec(), dict(VQ, vq_ema=False), 'step', ''),
    'vq_ema': (tiny_spec(), dict(VQ, vq_ema=True), 'step', ''),
    'parts_tiny': (tiny_spec(), {}, 'parts', 'lat_block gauss_head'),
    'parts_neck128': (neck_spec(5, 128), {}, 'parts', 'neck lat_block fused_tail'),
    'parts_neck256': (neck_spec(5, 256), {}, 'parts', 'neck lat_block fused_tail'),
    'parts_vq': (tiny_spec(), dict(VQ, vq_ema=False), 'parts', ''),
    'parts_vq_ema': (tiny_spec(), dict(VQ, vq_ema=True), 'parts', ''),
    'parts_separate': (DENSE1, {}, 'parts', ''),
}


def run_case(bk, name):
  """-> (engine, [[name, argument ...]] of every library call from construction on)"""
  spec, kw, run, _ = CASES[name]
  calls = []
  eng = VAEEngine(*spec, 4, bk.dev, lib=Recorder(bk.L, calls, args=True), **kw)
  x, eps = case_data(bk.dev, spec)
  if run.startswith('step'):
    for _ in range(1 + (run == 'step2')):
      eng.train_step(x, eps, lr=1e-3, beta=2.0, capacity=0.5 if eng.capacity_on else None)
    return eng, calls
  eng.step_count = 1
  eng.set_hyper(beta=2.0)
  if run == 'unfused':
    eng.forward(x, eps, fused=False)
    eng.backward()
  else:
    _, z = eng.run_encoder(x, eps)
    eng.observation_llk(eng.run_decoder(z), x, eng.llk)
  return eng, calls


@pytest.fixture(scope='module')
def golden():
  with open(GOLDEN) as f:
    return json.load(f)


@pytest.mark.parametrize('name', sorted(CASES))
def test_calls_match_the_record(bk, golden, name):
  eng, calls = run_case(bk, name)
  # (the path the case is there for: a fixture must not silently record another one)
  assert ' '.join(f for f in FLAGS if (getattr(eng, f)() if f == '_bwd_neck' else getattr(eng, f))) == CASES[name][3]
  want = golden[name]
  assert [c[0] for c in calls] == [c[0] for c in want]
  for i, (got, exp) in enumerate(zip(json.loads(json.dumps(calls)), want)):
    if bk.name == 'hip' and _lib.SIGNATURES[got[0]][-1:] == [_lib.P]:
      got, exp = got[:-1], exp[:-1]   # (the stream: set on the GPU outside the dry runs, null on the simulator)
    assert got == exp, (i, got, exp)


def test_failed_weight_gradient_leaves_no_open_bracket():
  """odin_conv2d_wgrad fails once between odin_wgrad_pair_begin and _end of the neck's backward pass: the step after it
  computes what a fresh engine computes (host-side error handling: the simulator only)"""
  from tests.simutil import sim_lib
  sim = sim_lib()

  class FailOnce:
    armed = failed = False
    open_pairs = 0

    def __getattr__(self, name):
      fn = getattr(sim, name)

      def call(*a):
        self.open_pairs += (name == 'odin_wgrad_pair_begin') - (name == 'odin_wgrad_pair_end')
        if name == 'odin_wgrad_pair_begin':
          self.armed = not self.failed
        if name == 'odin_conv2d_wgrad' and self.armed:
          self.armed, self.failed = False, True
          raise OdinError('odin_conv2d_wgrad failed: injected')
        return fn(*a)
      return call if name.startswith('odin_') else fn
  spec = neck_spec(5, 128)
  x, eps = case_data('cpu', spec)
  grads = []
  for L in (FailOnce(), sim):
    eng = VAEEngine(*spec, 4, 'cpu', lib=L)
    eng._neck_bwd_opt = True
    g = torch.Generator().manual_seed(0)
    p0 = torch.randn(eng.params.numel(), generator=g) * 0.1
    eng.params.copy_(p0)
    if L is not sim:
      with pytest.raises(OdinError, match='injected'):
        eng.train_step(x, eps, lr=1e-3, beta=2.0)
      assert L.failed and L.open_pairs == 0
      eng.params.copy_(p0)
    eng.train_step(x, eps, lr=1e-3, beta=2.0)
    assert eng._bwd_neck()
    grads.append(eng.grads.clone())
  assert torch.equal(grads[0], grads[1]) and float(grads[0].abs().max()) > 0
