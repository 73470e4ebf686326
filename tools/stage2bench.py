#!/usr/bin/env python3
"""TwoStageVAE's second stage on the GPU (stage2.hip), at B = 256, D = 10, units (1024,) * 3 by default:

  heads   each skip head against the project's own route in the same call: a device copy of [x | h] into a [B, K] buffer,
          odin_dense_fwd / odin_dense_bwd over it (they take any K: K' = K), the Gaussian likelihood launch
          (odin_elbo_gaussian_fwd_bwd at one pixel: the nearest pass the library has) and, backwards, the copy of the
          hidden part out of the concatenated gradient (its act' is left out: the route is not charged for it)
  steps   `--steps n`: n eager stage-2 steps of the model (run under rocprofv3 --kernel-trace for the per-kernel times)

usage: tools/stage2bench.py [--B 256] [--D 10] [--H 1024] [--steps 0]"""
import argparse
import ctypes as C
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from odin_ai_amd import _lib

ap = argparse.ArgumentParser()
ap.add_argument('--B', type=int, default=256)
ap.add_argument('--D', type=int, default=10)
ap.add_argument('--H', type=int, default=1024)
ap.add_argument('--steps', type=int, default=0)
args = ap.parse_args()
L = _lib.load()
dev = torch.device('cuda:0')


def t(fn, n=300):
  for _ in range(30):
    fn()
  torch.cuda.synchronize()
  e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
  e0.record()
  for _ in range(n):
    fn()
  e1.record()
  torch.cuda.synchronize()
  return e0.elapsed_time(e1) / n * 1e3


if args.steps > 0:
  from odin_ai_amd.networks import get_networks
  from odin_ai_amd.vae import TwoStageVAE
  vae = TwoStageVAE(device=dev, stage2_units=(args.H,) * 3, **get_networks('dsprites', zdim=args.D)).set_train_stage(2)
  x = (torch.rand(args.B, 64, 64, 1, device=dev) < 0.2).float()
  for _ in range(5):
    vae.optimize(x)
  torch.cuda.synchronize()
  us = t(lambda: vae.optimize(x), n=args.steps)
  print(f'stage-2 step (eager, first-stage encoder included) B={args.B} D={args.D} units=({args.H},)*3: {us:.1f} us')
  sys.exit(0)

B, D, H = args.B, args.D, args.H
E, N, K = D, 2 * D, D + H
st = torch.cuda.current_stream().cuda_stream
x, h = torch.randn(B, D, device=dev), torch.relu(torch.randn(B, H, device=dev))
w, b = torch.randn(K, N, device=dev) / K ** 0.5, torch.randn(N, device=dev)
tgt, scale = torch.randn(B, E, device=dev), torch.full((1,), 1.0 / B, device=dev)
p, dp, llk = torch.empty(B, N, device=dev), torch.empty(B, N, device=dev), torch.empty(B, device=dev)
dh, dx = torch.empty(B, H, device=dev), torch.empty(B, D, device=dev)
word = torch.zeros(2048, dtype=torch.int32, device=dev)
rows = C.c_int(0)
L.odin_skip_head_bwd(None, None, None, None, 2, None, None, None, None, C.byref(rows), B, D, H, N, None)
slab = torch.empty(rows.value, K * N + N, device=dev)
P = lambda a: a.data_ptr()

f0 = t(lambda: L.odin_skip_head_fwd(P(x), P(h), P(w), P(b), P(p), 0, None, None, None, None, B, D, H, N, st))
f1 = t(lambda: L.odin_skip_head_fwd(P(x), P(h), P(w), P(b), P(p), 1, P(tgt), P(scale), P(llk), P(dp), B, D, H, N, st))
bw = t(lambda: L.odin_skip_head_bwd(P(x), P(h), P(w), P(dp), 2, P(dh), P(word), P(dx), P(slab), C.byref(rows), B, D, H, N, st))
print(f'B={B} Dx={D} H={H} N={N}: skip_head_fwd mode 0 {f0:.2f} us, mode 1 {f1:.2f} us, skip_head_bwd {bw:.2f} us '
      f'({rows.value} slab rows)')

# the project's own route over a materialised concatenation
cat, dcat = torch.empty(B, K, device=dev), torch.empty(B, K, device=dev)
npart = C.c_int(0)
L.odin_elbo_gaussian_fwd_bwd(None, None, None, None, None, B, 1, E, 1, C.byref(npart), None)
part = torch.empty(B * max(npart.value, 1), device=dev)
wrows, crows = C.c_int(0), C.c_int(0)
L.odin_dense_wgrad(None, None, None, C.byref(wrows), B, K, N, None)
wslab = torch.empty(max(wrows.value, 1), K * N + N, device=dev)


def copy_in():
  cat[:, :D].copy_(x)
  cat[:, D:].copy_(h)


try:
  c = t(copy_in)
  g = t(lambda: L.odin_dense_fwd(P(cat), P(w), P(b), P(p), B, K, N, 0, st))
  path_f = L.odin_debug_last_path().decode()
  e = t(lambda: L.odin_elbo_gaussian_fwd_bwd(P(p), P(tgt), P(part), P(dp), P(scale), B, 1, E, 1, C.byref(npart), st))
  d = t(lambda: L.odin_dense_bwd(P(cat), P(dp), P(w), None, 0, P(dcat), None, C.byref(crows), P(wslab), C.byref(wrows),
                                 B, K, N, 1, 1, None, None, st))
  path_b = L.odin_debug_last_path().decode()
  o = t(lambda: dh.copy_(dcat[:, D:]))
  print(f'route: copy in {c:.2f} us + odin_dense_fwd {g:.2f} us [{path_f}] = {c + g:.2f} us (mode 0); '
        f'+ Gaussian pass {e:.2f} us = {c + g + e:.2f} us (mode 1)')
  print(f'route backward: odin_dense_bwd {d:.2f} us [{path_b}, {wrows.value} slab rows] + copy out {o:.2f} us '
        f'(+ copy in {c:.2f} us when the forward did not keep it) = {d + o:.2f} us')
  print(f'heads / route: fwd mode 0 {f0 / (c + g):.2f}, fwd mode 1 {f1 / (c + g + e):.2f}, bwd {bw / (d + o):.2f}')
except _lib.OdinError as err:
  print(f'route: the dense kernels refuse K = {K}: {err}')
