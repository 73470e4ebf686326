"""InfoVAE's MMD and DIPVAE's penalty under data parallelism on CPU: two gloo ranks (kernel sources on the simulator)
== one rank on the global batch -- the MMD shard form (all-gather z | shard kernel | all-reduce of the value shares)
and the DIP moments / finish pair (moment blocks all-gathered), through the segmented step program, 1 and 2 gradient
buckets."""
import os
import sys

import numpy as np
import pytest
import torch
import torch.distributed as dist

from tests.dp_util import dp_data as _data, dp_init as _init, gloo_rank, two_ranks
from tests.engine_util import tiny_spec as _spec
from tests.simutil import sim_lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REG = dict(mmd=dict(latent_reg='mmd', reg_coef=5.0, mmd_prior_samples=11),
           dip_ii=dict(latent_reg='dip_ii', reg_coef=1.0, dip_lambda=(1.5, 2.5)))


def _run(eng, xs, es, world):
  from odin_ai_amd.dist import SegmentedGraph
  outs = []
  for _ in range(2):
    eng.step_count += 1
    eng.set_hyper(lr=1e-3, beta=2.0)
    sg = SegmentedGraph('cpu', eng.step_program(xs, es, (100.0, None, None, None, True)))
    sg.run_eager()
    outs.append(eng.out4.clone())
  return torch.stack(outs), ''.join(k for k, _ in sg.segs)


def _worker(rank, world, port, out_path, reg, buckets):
  sys.path.insert(0, ROOT)
  from odin_ai_amd.dist import shard_batch
  from odin_ai_amd.engine import VAEEngine
  L = gloo_rank(rank, world, port)
  enc, dec, shp, D = _spec()
  B = 8
  x, eps = _data(B)
  # (each rank its own engine seed, as bench.py and the model API give them; the prior seed is shared)
  eng = VAEEngine(enc, dec, shp, D, B // world, 'cpu', lib=L, world_size=world, seed=1 + rank, dp_buckets=buckets,
                  prior_seed=3, **REG[reg])
  _init(eng)
  out4, kinds = _run(eng, shard_batch(x, rank, world), shard_batch(eps, rank, world), world)
  if rank == 0:
    torch.save(dict(params=eng.params.clone(), out4=out4, kinds=kinds), out_path)
  dist.destroy_process_group()


@pytest.mark.parametrize('buckets', [1, 2])
@pytest.mark.parametrize('reg', sorted(REG))
def test_two_gloo_ranks_match_single_rank(tmp_path, reg, buckets):
  from odin_ai_amd.engine import VAEEngine
  L = sim_lib()
  r2 = two_ranks(tmp_path, _worker, reg, buckets)
  enc, dec, shp, D = _spec()
  x, eps = _data(8)
  eng = VAEEngine(enc, dec, shp, D, 8, 'cpu', lib=L, prior_seed=3, **REG[reg])
  _init(eng)
  out1, kinds1 = _run(eng, x, eps, 1)
  assert 'c' not in kinds1
  # MMD: (k | all-gather | shard | all-reduce | finalise ...); DIP: (k | all-gather | finish ...)
  assert r2['kinds'].count('c') >= 2
  assert float((out1[:, 3]).abs().min()) > 0
  # (out4[0:3] are rank 0's local means; the regulariser's term is the global batch's on every rank)
  np.testing.assert_allclose(r2['out4'][:, 3].numpy(), out1[:, 3].numpy(), rtol=2e-5, atol=2e-6)
  np.testing.assert_allclose(r2['params'].numpy(), eng.params.numpy(), rtol=0, atol=2e-6)
