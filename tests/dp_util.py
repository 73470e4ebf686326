"""Two gloo ranks on the simulator against one rank on the whole batch: what tests/test_dp_gloo.py and its kin share."""
import os
import socket

import torch

from odin_ai_amd import _lib
from tests.engine_util import tiny_batch


def dp_data(B):
  return tuple(torch.tensor(a) for a in tiny_batch(5, B))


def dp_init(eng):
  eng.params.copy_(torch.randn(eng.params.numel(), generator=torch.Generator().manual_seed(0)) * 0.1)


def gloo_rank(rank, world, port):
  """first thing in a spawned worker: joins the process group; -> the simulator library"""
  os.environ['MASTER_ADDR'] = '127.0.0.1'
  os.environ['MASTER_PORT'] = str(port)
  torch.distributed.init_process_group('gloo', rank=rank, world_size=world)
  return _lib.Lib(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'sim', 'libodin_sim.so'))


def two_ranks(tmp_path, worker, *args):
  """worker(rank, 2, port, out_path, *args) on two spawned gloo ranks; -> what rank 0 saved"""
  s = socket.socket()
  s.bind(('127.0.0.1', 0))
  port = s.getsockname()[1]
  s.close()
  out = str(tmp_path / 'rank0.pt')
  torch.multiprocessing.spawn(worker, args=(2, port, out) + args, nprocs=2, join=True)
  return torch.load(out)
