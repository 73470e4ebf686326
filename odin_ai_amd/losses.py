"""The latent regularisers of InfoVAE / DIPVAE as stand-alone, forward-only calls on a posterior
(odin/bay/vi/losses.py:39-98, 163-276).  Both run the HIP kernels of latent_reg.hip; inside a training step the
engine runs the same kernels with their backward (VAEEngine(latent_reg=...)).
"""
from __future__ import annotations

import functools
from typing import Optional, Tuple

import torch

from . import _lib
from .engine import MMD_KERNELS


def _lib_stream(t: torch.Tensor, lib):
  lib = lib if lib is not None else _lib.load()
  st = torch.cuda.current_stream(t.device).cuda_stream if t.device.type == 'cuda' else None
  return lib, st


def _prior_samples(p_sample_shape) -> int:
  if isinstance(p_sample_shape, int):
    return int(p_sample_shape)
  shp = tuple(p_sample_shape)
  if len(shp) != 1:
    raise NotImplementedError(f'p_sample_shape={p_sample_shape!r}: one sample axis on the HIP path')
  return int(shp[0])


def _check_kernel(kernel: str) -> int:
  if kernel == 'polynomial':
    raise NotImplementedError('polynomial_kernel is not implemented (the reference raises here too, losses.py:219)')
  if kernel not in MMD_KERNELS:
    raise NotImplementedError("No support for kernel: '%s'" % kernel)
  return MMD_KERNELS[kernel]


def maximum_mean_discrepancy(qZ, pZ=None, q_sample_shape=(), p_sample_shape=100, kernel: str = 'gaussian',
                             seed: int = 1, y: Optional[torch.Tensor] = None, lib=None) -> torch.Tensor:
  """losses.py:222-276: mean k(x,x) + mean k(y,y) - 2 mean k(x,y) between samples x of qZ (an MVNDiagPosterior) and
  y of the prior N(0, I) -- one launch of odin_mmd_fwd_bwd, forward only.  q_sample_shape=None reuses qZ's cached
  sample, () draws one fresh sample; y: an explicit prior sample [M, D], otherwise M = p_sample_shape rows are drawn
  on the device from the Philox stream keyed by `seed`.  Returns a 0-d tensor."""
  k = _check_kernel(kernel)
  if q_sample_shape is None:
    x = qZ.z
  elif isinstance(q_sample_shape, (tuple, list)) and len(q_sample_shape) == 0:
    x = qZ.sample()
  else:
    raise NotImplementedError(f'q_sample_shape={q_sample_shape!r}: MMD on fresh posterior samples of a sample shape '
                              f'is not supported on the HIP path (q_sample_shape=None or ())')
  x = x.reshape(-1, x.shape[-1]).to(torch.float32).contiguous()
  N, D = x.shape
  if y is not None:
    y = y.reshape(-1, D).to(device=x.device, dtype=torch.float32).contiguous()
  M = y.shape[0] if y is not None else _prior_samples(p_sample_shape)
  lib, st = _lib_stream(x, lib)
  ws = torch.zeros(lib.odin_mmd_workspace(N, N, M, D), dtype=torch.float32, device=x.device)
  lib.odin_mmd_fwd_bwd(x.data_ptr(), y.data_ptr() if y is not None else None, ws.data_ptr(), None, None, None,
                       N, M, D, k, int(seed), None, st)
  return ws[0].clone()


def disentangled_inferred_prior_loss(qZ_X, only_mean: bool = False, lambda_offdiag: float = 2.,
                                     lambda_diag: float = 1., lib=None) -> torch.Tensor:
  """losses.py:39-98: lambda_offdiag * sum_{k!=l} Cov_kl^2 + lambda_diag * sum_k (Cov_kk - 1)^2 with Cov the
  covariance of the posterior means (+ E[diag(scale^2)] unless only_mean) -- one launch of odin_dip_fwd_bwd, forward
  only.  Returns a 0-d tensor."""
  p = torch.cat([qZ_X.loc, qZ_X.raw_scale], dim=-1)
  D = qZ_X.loc.shape[-1]
  p = p.reshape(-1, 2 * D).to(torch.float32).contiguous()
  lib, st = _lib_stream(p, lib)
  ws = torch.zeros(lib.odin_dip_workspace(1, D), dtype=torch.float32, device=p.device)
  lib.odin_dip_fwd_bwd(p.data_ptr(), ws.data_ptr(), None, None, None, None, p.shape[0], D, int(not only_mean),
                       float(lambda_diag), float(lambda_offdiag), st)
  return ws[0].clone()


def mmd_config(divergence) -> Tuple[str, int]:
  """InfoVAE's `divergence`: a functools.partial of maximum_mean_discrepancy (this module's, or the reference's
  of the same name) -> (kernel, p_sample_shape).  Everything the HIP path does not compute raises."""
  if not isinstance(divergence, functools.partial) or getattr(divergence.func, '__name__', '') != \
      'maximum_mean_discrepancy':
    raise NotImplementedError(f'divergence={divergence!r}: the HIP path computes InfoVAE\'s divergence only as '
                              f'functools.partial(maximum_mean_discrepancy, ...)')
  if divergence.args:
    raise NotImplementedError('divergence: positional arguments bound in the partial are not supported')
  kw = dict(divergence.keywords)
  unknown = set(kw) - {'kernel', 'q_sample_shape', 'p_sample_shape'}
  if unknown:
    raise NotImplementedError(f'divergence: unsupported arguments {sorted(unknown)}')
  q = kw.get('q_sample_shape', ())
  if q is not None:
    raise NotImplementedError(f'divergence: q_sample_shape={q!r} -- MMD on fresh posterior samples is not supported '
                              f'on the HIP path; q_sample_shape=None reuses the forward\'s sample')
  kernel = kw.get('kernel', 'gaussian')
  _check_kernel(kernel)
  return kernel, _prior_samples(kw.get('p_sample_shape', 100))
