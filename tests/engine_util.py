"""Scaffolding shared by the engine tests: the tiny network specs and the recorder of library calls."""
import ctypes as C

import numpy as np
import torch

from odin_ai_amd import _lib
from odin_ai_amd.engine import VAEEngine

_ENC = [('center',), ('conv', 8, 4, 2, 'elu'), ('conv', 16, 4, 2, 'elu'), ('flatten',), ('dense', 24, 'linear')]


def tiny_spec(zdim=4, C=1):
  """8 x 8 x C: two convolutions | latent block | two Conv2DTranspose and a 1x1 head"""
  dec = [('dense', 32, 'linear'), ('reshape', (2, 2, 8)), ('deconv', 16, 4, 2, 'elu'), ('deconv', 8, 4, 2, 'elu'),
         ('conv', C, 1, 1, 'linear')]
  return list(_ENC), dec, (8, 8, C), zdim


def tiny16_spec(C=1, zdim=5):
  """16 x 16 x C: the last two decoder layers run as the fused Bernoulli tail"""
  dec = [('dense', 128, 'linear'), ('reshape', (4, 4, 8)), ('deconv', 16, 4, 2, 'elu'), ('deconv', 8, 4, 2, 'elu'),
         ('conv', C, 1, 1, 'linear')]
  return list(_ENC), dec, (16, 16, C), zdim


def neck_spec(zdim=5, proj=128, C=1):
  """the neck of the dSprites / Shapes3D stacks (image_networks.py:466-471, 494-502) under a shortened encoder / decoder:
  ... -> [8, 8, 64] -> Conv2D(64, 4, 2) -> Flatten -> Dense(proj) | Dense(proj) -> (4, 4, proj / 16) -> deconv 64 -> ..."""
  enc = [('center',), ('conv', 64, 4, 2, 'elu'), ('conv', 64, 4, 2, 'elu'), ('flatten',), ('dense', proj, 'linear')]
  dec = [('dense', proj, 'linear'), ('reshape', (4, 4, proj // 16)), ('deconv', 64, 4, 2, 'elu'),
         ('deconv', 8, 4, 2, 'elu'), ('conv', C, 1, 1, 'linear')]
  return enc, dec, (16, 16, C), zdim


def tiny_nets(C=1, zdim=4, hw=8):
  """tiny_spec as the model API's keyword arguments"""
  from odin_ai_amd.networks import RVconf, SequentialNetwork
  enc, dec, _, _ = tiny_spec(zdim, C)
  return dict(encoder=SequentialNetwork(enc, 'Encoder', (hw, hw, C)), decoder=SequentialNetwork(dec, 'Decoder', (zdim,)),
              observation=RVconf((hw, hw, C), 'bernoulli', projection=False, name='image'),
              latents=RVconf((zdim,), 'mvndiag', projection=True, name='latents'))


def head_spec(maps, zdim=4, C=1):
  """tiny_spec with a 1x1 head of `maps` maps (the Gaussian and the logistic observations)"""
  e, d, s, z = tiny_spec(zdim, C)
  return e, d[:-1] + [('conv', maps, 1, 1, 'linear')], s, z


def dense_spec(hw=8):
  """Dense layers only: the stand-alone Bernoulli kernel keeps the top range word"""
  return ([('flatten',), ('dense', 40, 'relu'), ('dense', 24, 'relu')],
          [('dense', 24, 'relu'), ('dense', hw * hw, 'linear'), ('reshape', (hw, hw, 1))], (hw, hw, 1), 4)


def _struct(s):
  """a ctypes structure as a list: its numbers, and for every pointer only whether it is set"""
  return [getattr(s, n) is not None if t is C.c_void_p else getattr(s, n) for n, t in s._fields_ if n != 'pad_']


def _arg(t, a):
  if isinstance(a, C.Array):                 # the reduction jobs: (is the source set, is the target set, n, rows, stride)
    return [_struct(j) for j in a]
  if hasattr(a, '_obj'):                     # byref(...): a descriptor's contents; of an output word only that it is there
    return _struct(a._obj) if isinstance(a._obj, C.Structure) else True
  return a is not None if (t is _lib.P or a is None) else a


class Recorder:
  """A kernel library whose odin_* calls are appended to `calls` on their way through (hand it to VAEEngine as `lib`):
  the call's name or, with `args`, [name, argument ...] -- numbers as they are, of a pointer only whether it is null
  (_lib.SIGNATURES says which is which, the trailing stream included), structures field by field."""

  def __init__(self, L, calls, args=False):
    self._L, self.calls, self.args = L, calls, args

  def __getattr__(self, name):
    fn = getattr(self._L, name)
    if not name.startswith('odin_'):
      return fn
    sig = _lib.SIGNATURES[name]

    def call(*a):
      self.calls.append([name] + [_arg(t, v) for t, v in zip(sig, a)] if self.args else name)
      return fn(*a)
    return call


def case_data(dev, spec, B=4):
  """-> (x in (0, 1), eps) for a spec on a device, the same at every call"""
  rng = np.random.default_rng(3)
  return tuple(torch.tensor(a, dtype=torch.float32, device=dev)
               for a in (np.clip(rng.random((B,) + spec[2]), 1e-6, 1 - 1e-6), rng.standard_normal((B, spec[3]))))


def launch_record(bk, steps=1, **kw):
  """train_steps of a tiny_spec() engine; -> (engine, the names of every library call of the LAST step, in order)"""
  calls = []
  eng = VAEEngine(*tiny_spec(), 4, bk.dev, lib=Recorder(bk.L, calls), **kw)
  x, eps = case_data(bk.dev, tiny_spec())
  for _ in range(steps):
    calls.clear()
    eng.train_step(x, eps, lr=1e-3, beta=2.0)
  return eng, calls


def tiny_batch(seed, B=6, D=4, C=1):
  """-> float32 (x in (0, 1) of [B, 8, 8, C], eps of [B, D])"""
  rng = np.random.default_rng(seed)
  x = np.clip(rng.random((B, 8, 8, C)), 1e-6, 1 - 1e-6).astype(np.float32)
  return x, rng.standard_normal((B, D)).astype(np.float32)


def factor_batch(seed, B1=4, D=4):
  """FactorVAE's step inputs: -> (x of [2 B1, 8, 8, 1], eps and eps2 of [B1, D], a permutation of the batch per latent)"""
  rng = np.random.default_rng(seed)
  x = np.clip(rng.random((2 * B1, 8, 8, 1)), 1e-6, 1 - 1e-6).astype(np.float32)
  eps, eps2 = (rng.standard_normal((B1, D)).astype(np.float32) for _ in range(2))
  return x, eps, eps2, np.stack([rng.permutation(B1) for _ in range(D)], 1).astype(np.int32)
