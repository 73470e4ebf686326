"""VariationalAutoencoder / BetaVAE / AnnealingVAE / BetaTCVAE / FactorVAE / InfoVAE / DIPVAE / TwoStageVAE on the HIP engine.

Drop-in for the reference's model API on this path (same class names, constructor
arguments, method names, returned structures and error behaviour):

  odin/bay/vi/autoencoder/variational_autoencoder.py:132 (VariationalAutoencoder, VAEStep)
  odin/bay/vi/_base.py:21-194                             (ELBO configuration, elbo())
  odin/bay/vi/autoencoder/beta_vae.py:11,83,110           (BetaVAE, AnnealingVAE, BetaTCVAE)
  odin/bay/vi/autoencoder/factor_vae.py:99                (FactorVAE, two-step training)
  odin/bay/vi/autoencoder/info_vae.py:28-91               (InfoVAE: maximum-mean discrepancy)
  odin/bay/vi/autoencoder/dip_vae.py                      (DIPVAE: disentangled inferred prior)
  odin/bay/vi/autoencoder/two_stage_vae.py                (TwoStageVAE: a second VAE over the latents)
  odin/bay/vi/autoencoder/multitask_vae.py                (MultitaskVAE / SkiptaskVAE: a label head on the latents)
  odin/networks/base_networks.py:415-812                  (optimize(), fit())
  odin/bay/layers/continuous.py:459-483                   (latent posteriors 'mvndiag' and 'mvntril')
  odin/bay/layers/discrete.py:286-343                     (latent posterior 'relaxedonehot' / 'relaxedsoftmax')
  odin/bay/layers/discrete.py:346 ff.                     (latent posterior 'relaxedbern' / 'relaxedsigmoid' / 'relaxedbernoulli')

Tensors are torch tensors on the model's device; returned "distributions" are light
objects exposing what callers of the reference use (mean / stddev / sample / log_prob /
event_shape / batch_shape / KL_divergence).  Every FLOP of encode / decode / ELBO /
backward / Adam runs in libodin_hip.so through ``VAEEngine``.
"""
from __future__ import annotations

import ctypes as C
import functools
import math
import os
from dataclasses import dataclass, field
from typing import Any, Callable, Dict, Iterator, List, Optional, Sequence, Tuple, Union

import numpy as np
import torch

from . import _lib
from .engine import (ACT, H_ALPHA, N_HYPER, RANGE_WORDS, NetProgram, ParamLayout, ReduceJob, VAEEngine,
                     build_layers)
from .interpolation import Interpolation, linear
from .losses import disentangled_inferred_prior_loss, maximum_mean_discrepancy, mmd_config
from .networks import RVconf, SequentialNetwork, get_networks, layer_names

LOG2PI = math.log(2.0 * math.pi)


# ======================================================================================
# light distribution objects
# ======================================================================================
class KLdivergence:
  """odin/bay/helpers.py:285-372: callable attached to the posterior; `.prior` attribute."""

  def __init__(self, posterior: 'MVNDiagPosterior', prior='Independent(Normal(0,1))'):
    self.posterior, self.prior = posterior, prior

  def __call__(self, analytic=False, reverse=True, free_bits=None, sample_shape=None,
               keepdims=False):
    q = self.posterior
    if not reverse and not analytic:
      raise TypeError('reverse=False needs analytic=True (helpers.py:261-276: the swapped '
                      '"posterior" is the prior, which carries no cached sample)')
    if isinstance(q, MVNTriLPosterior):
      return self._tril(q, analytic, reverse, free_bits, keepdims)
    if isinstance(q, RelaxedOneHotPosterior):
      return self._concrete(q, analytic, reverse, free_bits, keepdims)
    if isinstance(q, RelaxedBernoulliPosterior):
      return self._relaxedbern(q, analytic, reverse, free_bits, keepdims)
    if not reverse:  # KL(p || q), helpers.py:261-265
      kl = (torch.log(q.scale) + 0.5 * (1.0 + q.loc ** 2) / q.scale ** 2 - 0.5).sum(-1)
    elif analytic:
      kl = 0.5 * (q.scale ** 2 + q.loc ** 2 - 1.0 - 2.0 * torch.log(q.scale)).sum(-1)
    else:
      z = q.z
      lq = (-0.5 * ((z - q.loc) / q.scale) ** 2 - torch.log(q.scale)).sum(-1)
      lp = (-0.5 * z ** 2).sum(-1)
      kl = lq - lp
    if free_bits is not None:
      kl = torch.clamp(kl, min=free_bits * q.loc.shape[-1])
    if analytic and keepdims:
      kl = kl.unsqueeze(0)  # odin/bay/helpers.py:370-371
    return kl

  @staticmethod
  def _tril(q: 'MVNTriLPosterior', analytic, reverse, free_bits, keepdims):
    if not reverse:
      raise NotImplementedError("'mvntril' with reverse=False: KL(p || q) needs the inverse of L")
    D = q.loc.shape[-1]
    logdet = torch.log(torch.diagonal(q.scale_tril, dim1=-2, dim2=-1)).sum(-1)
    if analytic:
      # (TFP registers no KL between MultivariateNormalTriL and Independent(Normal): the closed form is the evident
      # intent -- DESIGN 3.15)
      kl = 0.5 * ((q.scale_tril ** 2).sum((-2, -1)) + (q.loc ** 2).sum(-1) - D) - logdet
    else:
      kl = q.log_prob(q.z) - (-0.5 * (q.z ** 2).sum(-1) - 0.5 * D * LOG2PI)
    if free_bits is not None:
      kl = torch.clamp(kl, min=free_bits * D)
    if analytic and keepdims:
      kl = kl.unsqueeze(0)
    return kl


  @staticmethod
  def _concrete(q: 'RelaxedOneHotPosterior', analytic, reverse, free_bits, keepdims):
    if not reverse:
      raise NotImplementedError(CONCRETE_NO_FORWARD_KL)
    K = q.logits.shape[-1]
    if analytic:
      # (TFP registers no KL between RelaxedOneHotCategorical and OneHotCategorical: the categorical KL of Jang et al.
      # against the uniform prior -- DESIGN 3.16)
      lp = torch.log_softmax(q.logits, -1)
      kl = (lp.exp() * (lp + math.log(K))).sum(-1)
    else:
      kl = q.log_prob_cached() + math.log(K) * q.z.sum(-1)
    if free_bits is not None:
      kl = torch.clamp(kl, min=free_bits * K)
    if analytic and keepdims:
      kl = kl.unsqueeze(0)
    return kl

  @staticmethod
  def _relaxedbern(q: 'RelaxedBernoulliPosterior', analytic, reverse, free_bits, keepdims):
    if not reverse:
      raise NotImplementedError(RELAXEDBERN_NO_FORWARD_KL)
    D = q.logits.shape[-1]
    if analytic:
      # (TFP registers no KL between RelaxedBernoulli and Bernoulli: the Bernoulli KL of Jang et al. against the
      # prior of probability 1/2, per unit t tanh t - log cosh t with t = logits / 2 -- DESIGN 3.18)
      t = 0.5 * q.logits.abs()
      th, e = torch.tanh(t), torch.exp(-2.0 * t)
      # (near 0 the second form is a difference of terms near log 2; above 1 the first one's 1 - tanh^2 cancels)
      kl = torch.where(t < 1.0, t * th + 0.5 * torch.log1p(-th * th),
                       math.log(2.0) - torch.log1p(e) - 2.0 * t * e / (1.0 + e)).sum(-1)
    else:
      kl = q.log_prob_cached() + D * math.log(2.0)
    if free_bits is not None:
      kl = torch.clamp(kl, min=free_bits * D)
    if analytic and keepdims:
      kl = kl.unsqueeze(0)
    return kl


class MVNDiagPosterior:
  """MultivariateNormalDiag(loc, softplus(raw)) with its cached sample
  (odin/bay/layers/continuous.py:459-483; dense_distribution.py:339-380)."""

  def __init__(self, p: torch.Tensor, z: torch.Tensor, D: int):
    self.loc = p[:, :D]
    self.raw_scale = p[:, D:]
    self.scale = torch.nn.functional.softplus(self.raw_scale)
    self.z = z
    self.KL_divergence = KLdivergence(self)

  event_shape = property(lambda self: (self.loc.shape[-1],))
  batch_shape = property(lambda self: tuple(self.loc.shape[:-1]))

  def mean(self):
    return self.loc

  def stddev(self):
    return self.scale

  def sample(self, n=None, seed=None):
    g = None
    if seed is not None:
      g = torch.Generator(device=self.loc.device).manual_seed(int(seed))
    shp = tuple(self.loc.shape) if n is None else (int(n),) + tuple(self.loc.shape)
    return self.loc + self.scale * torch.randn(shp, device=self.loc.device, generator=g)

  def log_prob(self, z):
    D = self.loc.shape[-1]
    return (-0.5 * ((z - self.loc) / self.scale) ** 2 - torch.log(self.scale)).sum(-1) \
        - 0.5 * D * LOG2PI

  def __array__(self):
    return self.z.detach().cpu().numpy()

  def tensor(self):
    """tf.convert_to_tensor(q): the cached sample."""
    return self.z


TRIL_DIAG_SHIFT = 1e-5   # FillScaleTriL's diag_shift (continuous.py:465-469)


def fill_scale_tril(r: torch.Tensor, D: int) -> torch.Tensor:
  """tfb.FillScaleTriL(diag_bijector=softplus, diag_shift=1e-5): r [..., D (D + 1) / 2] -> L [..., D, D].  r[D:] followed
  by r reversed are D * D values, read row-major as a D x D matrix of which the lower triangle is kept."""
  m = torch.cat([r[..., D:], torch.flip(r, dims=(-1,))], -1).reshape(tuple(r.shape[:-1]) + (D, D))
  d = torch.nn.functional.softplus(torch.diagonal(m, dim1=-2, dim2=-1)) + TRIL_DIAG_SHIFT
  return torch.tril(m, -1) + torch.diag_embed(d)


class MVNTriLPosterior:
  """MultivariateNormalTriL(loc, FillScaleTriL(raw)) with its cached sample (odin/bay/layers/continuous.py:459-474,
  covariance='tril'); p [B, D + D (D + 1) / 2] = (loc | raw)."""

  def __init__(self, p: torch.Tensor, z: torch.Tensor, D: int):
    self.loc = p[:, :D]
    self.raw_scale = p[:, D:]
    self.scale_tril = fill_scale_tril(self.raw_scale, D)
    self.z = z
    self.KL_divergence = KLdivergence(self)

  event_shape = property(lambda self: (self.loc.shape[-1],))
  batch_shape = property(lambda self: tuple(self.loc.shape[:-1]))

  def mean(self):
    return self.loc

  def stddev(self):
    """sqrt of the covariance's diagonal: the row norms of L"""
    return torch.sqrt((self.scale_tril ** 2).sum(-1))

  def covariance(self):
    return self.scale_tril @ self.scale_tril.transpose(-1, -2)

  def sample(self, n=None, seed=None):
    g = None
    if seed is not None:
      g = torch.Generator(device=self.loc.device).manual_seed(int(seed))
    shp = tuple(self.loc.shape) if n is None else (int(n),) + tuple(self.loc.shape)
    e = torch.randn(shp, device=self.loc.device, generator=g)
    return self.loc + (self.scale_tril @ e.unsqueeze(-1)).squeeze(-1)

  def log_prob(self, z):
    D = self.loc.shape[-1]
    d = (z - self.loc).unsqueeze(-1)
    L = self.scale_tril.expand(tuple(d.shape[:-2]) + (D, D))
    e = torch.linalg.solve_triangular(L, d, upper=False).squeeze(-1)   # (host-side solve: L e = z - loc)
    return -0.5 * (e ** 2).sum(-1) - torch.log(torch.diagonal(self.scale_tril, dim1=-2, dim2=-1)).sum(-1) \
        - 0.5 * D * LOG2PI

  def __array__(self):
    return self.z.detach().cpu().numpy()

  def tensor(self):
    """tf.convert_to_tensor(q): the cached sample."""
    return self.z


CONCRETE_NO_FORWARD_KL = ("'relaxedonehot' with reverse=False: KL(p || q) of a one-hot prior against a density on the "
                          'simplex is not defined')


class RelaxedOneHotPosterior:
  """RelaxedOneHotCategorical(temperature, logits) with its cached sample (odin/bay/layers/discrete.py:286-343): ONE
  K-way variable.  p [B, K] are the logits, g [B, K] the Gumbel noise the cached sample z = softmax((logits + g) / tau)
  was drawn with -- kept so that the cached sample's density is evaluated in y = log z without taking log(z), which
  underflows at low temperatures."""

  def __init__(self, p: torch.Tensor, z: torch.Tensor, g: torch.Tensor, temperature: float):
    self.logits = p
    self.temperature = float(temperature)
    self.z, self.noise = z, g
    self.KL_divergence = KLdivergence(self, prior='OneHotCategorical(logits=0)')

  event_shape = property(lambda self: (self.logits.shape[-1],))
  batch_shape = property(lambda self: tuple(self.logits.shape[:-1]))

  @property
  def probs(self):
    return torch.softmax(self.logits, -1)

  def mean(self):
    raise NotImplementedError('RelaxedOneHotCategorical has no closed-form mean (TFP raises too)')

  def _gumbel(self, shp, seed=None):
    g = None
    if seed is not None:
      g = torch.Generator(device=self.logits.device).manual_seed(int(seed))
    u = torch.rand(shp, device=self.logits.device, generator=g).clamp_(2.0 ** -25, 1.0 - 2.0 ** -24)
    return -torch.log(-torch.log(u))

  def sample(self, n=None, seed=None):
    shp = tuple(self.logits.shape) if n is None else (int(n),) + tuple(self.logits.shape)
    return torch.softmax((self.logits + self._gumbel(shp, seed)) / self.temperature, -1)

  def _log_prob_y(self, y):
    K, tau = self.logits.shape[-1], self.temperature
    return (math.lgamma(K) + (K - 1) * math.log(tau)
            + torch.log_softmax(self.logits - tau * y, -1).sum(-1) - y.sum(-1))

  def log_prob(self, z):
    """the density on the simplex at any z (its logarithm is taken: entries that underflowed to 0 are held at the
    smallest normal float)"""
    return self._log_prob_y(torch.log(torch.clamp(z, min=torch.finfo(z.dtype).tiny)))

  def log_prob_cached(self):
    """log q(z) at the cached sample, from its noise: y = log_softmax((logits + g) / tau)"""
    return self._log_prob_y(torch.log_softmax((self.logits + self.noise) / self.temperature, -1))

  def __array__(self):
    return self.z.detach().cpu().numpy()

  def tensor(self):
    """tf.convert_to_tensor(q): the cached sample."""
    return self.z


RELAXEDBERN_NO_FORWARD_KL = ("'relaxedbernoulli' with reverse=False: KL(p || q) of a Bernoulli prior against a density "
                             'on the open unit cube is not defined')


def _softplus_pair(x):
  """softplus(x) + softplus(-x) = |x| + 2 log1p(exp(-|x|))"""
  ax = x.abs()
  return ax + 2.0 * torch.log1p(torch.exp(-ax))


class RelaxedBernoulliPosterior:
  """RelaxedBernoulli(temperature, logits) with its cached sample (odin/bay/layers/discrete.py:346 ff.): D independent
  binary-concrete units.  p [B, D] are the logits, n [B, D] the logistic noise the cached sample
  z = sigmoid((logits + n) / tau) was drawn with -- kept so that the cached sample's density is evaluated in
  u = (logits + n) / tau without taking logit(z): z rounds to exactly 0 or 1 at low temperatures."""

  def __init__(self, p: torch.Tensor, z: torch.Tensor, n: torch.Tensor, temperature: float):
    self.logits = p
    self.temperature = float(temperature)
    self.z, self.noise = z, n
    self.KL_divergence = KLdivergence(self, prior='Independent(Bernoulli(logits=0))')

  event_shape = property(lambda self: (self.logits.shape[-1],))
  batch_shape = property(lambda self: tuple(self.logits.shape[:-1]))

  @property
  def probs(self):
    return torch.sigmoid(self.logits)

  def mean(self):
    raise NotImplementedError('RelaxedBernoulli has no closed-form mean (TFP raises too)')

  def _logistic(self, shp, seed=None):
    g = None
    if seed is not None:
      g = torch.Generator(device=self.logits.device).manual_seed(int(seed))
    u = torch.rand(shp, device=self.logits.device, generator=g).clamp_(2.0 ** -25, 1.0 - 2.0 ** -24)
    return torch.log(u) - torch.log1p(-u)

  def sample(self, n=None, seed=None):
    shp = tuple(self.logits.shape) if n is None else (int(n),) + tuple(self.logits.shape)
    return torch.sigmoid((self.logits + self._logistic(shp, seed)) / self.temperature)

  def _log_prob_u(self, u, noise):
    """Logistic(logits / tau, 1 / tau).log_prob(u) pushed through Sigmoid; `noise` is its standardised argument
    tau u - logits"""
    return (math.log(self.temperature) + _softplus_pair(u) - _softplus_pair(noise)).sum(-1)

  def log_prob(self, z):
    """the density on the unit cube at z.  The cached sample itself (`q.tensor()`) is evaluated from its noise; at any
    other z the logit is taken, with entries that rounded to 0 or 1 held one step inside the interval."""
    if z is self.z:
      return self.log_prob_cached()
    fi = torch.finfo(z.dtype)
    zc = torch.clamp(z, min=fi.tiny, max=1.0 - fi.eps / 2)
    u = torch.log(zc) - torch.log1p(-zc)
    return self._log_prob_u(u, self.temperature * u - self.logits)

  def log_prob_cached(self):
    """log q(z) at the cached sample, from its noise: u = (logits + n) / tau"""
    return self._log_prob_u((self.logits + self.noise) / self.temperature, self.noise)

  def __array__(self):
    return self.z.detach().cpu().numpy()

  def tensor(self):
    """tf.convert_to_tensor(q): the cached sample."""
    return self.z


class BernoulliObservation:
  """Independent(Bernoulli(logits), 3) (odin/networks/image_networks.py:87-93)."""

  def __init__(self, logits: torch.Tensor):
    self.logits = logits

  event_shape = property(lambda self: tuple(self.logits.shape[1:]))
  batch_shape = property(lambda self: (self.logits.shape[0],))

  def mean(self):
    return torch.sigmoid(self.logits)

  def log_prob(self, x):
    e = x * self.logits - torch.nn.functional.softplus(self.logits)
    return e.reshape(e.shape[0], -1).sum(1)

  def sample(self, n=None):
    p = self.mean()
    if n is not None:
      p = p.unsqueeze(0).expand((int(n),) + tuple(p.shape))
    return torch.bernoulli(p)


class ContinuousBernoulliObservation:
  """Independent(ContinuousBernoulli(logits), 3) ('cbernoulli', odin/bay/distribution_alias.py:108;
  ContinuousBernoulliLayer, odin/bay/layers/discrete.py:82-121) in logit space, as the HIP kernel evaluates it:
  log p(x | l) = x l - A(l) with A(l) = log((e^l - 1) / l), mean mu = A'.  Below |l| = 1 both come from their five-term
  series (A(0) = 0 and mu(0) = 1/2 exactly), above it from the closed forms; the reference's `lims` band around
  probs = 1/2 has no counterpart."""
  SWITCH = 1.0

  def __init__(self, logits: torch.Tensor):
    self.logits = logits

  event_shape = property(lambda self: tuple(self.logits.shape[1:]))
  batch_shape = property(lambda self: (self.logits.shape[0],))
  probs = property(lambda self: torch.sigmoid(self.logits))

  def _parts(self):
    """(small, |l| with the small entries replaced by 1, l^2)"""
    l = self.logits
    a = l.abs()
    small = a < self.SWITCH
    return small, torch.where(small, torch.ones_like(a), a), l * l

  def log_normalizer(self):
    """A(l), elementwise"""
    l = self.logits
    small, a, l2 = self._parts()
    ser = 0.5 * l + l2 * (1 / 24 + l2 * (-1 / 2880 + l2 * (1 / 181440 - l2 / 9676800)))
    closed = torch.clamp(l, min=0) + torch.log1p(-torch.exp(-a)) - torch.log(a)
    return torch.where(small, ser, closed)

  def mean(self):
    l = self.logits
    small, a, l2 = self._parts()
    ser = 0.5 + l * (1 / 12 + l2 * (-1 / 720 + l2 * (1 / 30240 - l2 / 1209600)))
    e = torch.exp(-a)
    om = 1 - e
    r = 1 / (a * om)
    closed = torch.clamp(torch.where(l >= 0, a - om, om - a * e) * r, max=1.0)
    return torch.where(small, ser, closed)

  def log_prob(self, x):
    # as the kernel: above the switch x l - max(l, 0) is taken as (x - 1) l on the positive side, where the two terms
    # cancel (x = 1, l = 1e4: log p = 9.2 against terms of 1e4), and A(l) - max(l, 0) = log((1 - e^-|l|) / |l|)
    l = self.logits
    small, a, l2 = self._parts()
    ser = 0.5 * l + l2 * (1 / 24 + l2 * (-1 / 2880 + l2 * (1 / 181440 - l2 / 9676800)))
    rest = torch.log1p(-torch.exp(-a)) - torch.log(a)
    xx = torch.where(small | (l < 0), x, x - 1)
    e = xx * l - torch.where(small, ser, rest)
    return e.reshape(e.shape[0], -1).sum(1)

  def sample(self, n=None):
    """inverse CDF: x = 1 + log(u + (1 - u) e^-l) / l for l > 0, 1 - icdf(1 - u; -l) for l < 0, x = u at l = 0"""
    l = self.logits
    if n is not None:
      l = l.unsqueeze(0).expand((int(n),) + tuple(l.shape))
    u = torch.rand(l.shape, device=l.device, dtype=l.dtype)
    a = l.abs()
    flat = a < 1e-30
    a = torch.where(flat, torch.ones_like(a), a)
    v = torch.where(l >= 0, u, 1 - u)
    y = 1 + torch.log1p((1 - v) * torch.expm1(-a)) / a
    y = torch.where(l >= 0, y, 1 - y)
    return torch.where(flat, u, y).clamp(0.0, 1.0)


class NegativeBinomialObservation:
  """Independent(NegativeBinomial(total_count = exp(a), logits = l), 1) ('nb'; NegativeBinomialLayer with dispersion
  'full', odin/bay/layers/count_layers.py:75-163) over G genes: params [..., 2 G] = (a | l) = split(params, 2, axis=-1).
  `log_prob` runs the HIP kernel of the training step (odin_elbo_nb_fwd_bwd): lgamma(r + x) - lgamma(r) is
  formed as a difference there, which torch.lgamma in float32 cannot do."""
  PLANES = 2

  def __init__(self, params: torch.Tensor, lib=None):
    assert params.shape[-1] % self.PLANES == 0, params.shape
    self.params, self._lib = params, lib
    G = params.shape[-1] // self.PLANES
    self.log_total_count, self.logits = params[..., :G], params[..., G:2 * G]

  event_shape = property(lambda self: tuple(self.logits.shape[1:]))
  batch_shape = property(lambda self: (self.logits.shape[0],))
  total_count = property(lambda self: torch.exp(self.log_total_count))

  def mean(self):
    return torch.exp(self.log_total_count + self.logits)

  def log_prob(self, x):
    lib = self._lib if self._lib is not None else _lib.load()
    P, G = self.PLANES, self.logits.shape[-1]
    p = self.params.reshape(-1, P * G).to(torch.float32).contiguous()
    rows = p.shape[0]
    xx = torch.as_tensor(x, dtype=torch.float32, device=p.device).expand(self.logits.shape).reshape(rows, G).contiguous()
    st = torch.cuda.current_stream(p.device).cuda_stream if p.device.type == 'cuda' else None
    npart = C.c_int(0)
    lib.odin_elbo_nb_fwd_bwd(None, None, None, None, None, rows, G, P - 2, C.byref(npart), None, None)
    part, dp = torch.empty(rows * npart.value, dtype=torch.float32, device=p.device), torch.empty_like(p)
    out, one = torch.empty(rows, dtype=torch.float32, device=p.device), torch.ones(1, dtype=torch.float32, device=p.device)
    lib.odin_elbo_nb_fwd_bwd(p.data_ptr(), xx.data_ptr(), part.data_ptr(), dp.data_ptr(), one.data_ptr(), rows, G, P - 2,
                             C.byref(npart), None, st)
    lib.odin_sum_parts(part.data_ptr(), npart.value, out.data_ptr(), rows, st)
    return out.reshape(self.logits.shape[:-1])

  def sample(self, n=None):
    raise NotImplementedError(f'{type(self).__name__}.sample: sampling the count observations is not built')


class ZINegativeBinomialObservation(NegativeBinomialObservation):
  """ZeroInflated(NegativeBinomial(exp(a), logits = l), logits = pi) ('zinb'; ZINegativeBinomialLayer,
  count_layers.py:311-416; zero_inflated.py:216-230): params [..., 3 G] = (a | l | pi), pi the inflation logit; `rate` is
  the inflation probability sigmoid(pi)."""
  PLANES = 3

  def __init__(self, params: torch.Tensor, lib=None):
    super().__init__(params, lib)
    G = params.shape[-1] // 3
    self.inflation_logits = params[..., 2 * G:]

  rate = property(lambda self: torch.sigmoid(self.inflation_logits))

  def mean(self):
    return torch.sigmoid(-self.inflation_logits) * super().mean()


class GaussianObservation:
  """Independent(Normal(loc, scale), 3), params split on the channel axis
  (image_networks.py:95-102); softplus1 scale as GaussianLayer (continuous.py:196-260)."""

  def __init__(self, h: torch.Tensor, softplus1: bool):
    Cc = h.shape[-1] // 2
    self.loc = h[..., :Cc]
    raw = h[..., Cc:]
    self.scale = torch.nn.functional.softplus(raw + math.log(math.e - 1.0)) if softplus1 else raw

  event_shape = property(lambda self: tuple(self.loc.shape[1:]))
  batch_shape = property(lambda self: (self.loc.shape[0],))

  def mean(self):
    return self.loc

  def stddev(self):
    return self.scale

  def log_prob(self, x):
    e = -0.5 * ((x - self.loc) / self.scale) ** 2 - torch.log(self.scale) - 0.5 * LOG2PI
    return e.reshape(e.shape[0], -1).sum(1)

  def sample(self, n=None):
    shp = tuple(self.loc.shape) if n is None else (int(n),) + tuple(self.loc.shape)
    return self.loc + self.scale * torch.randn(shp, device=self.loc.device)


class QuantizedLogisticObservation:
  """QuantizedLogistic(loc, softplus(raw) + e^-7, low=0, high=255, inputs_domain='sigmoid',
  reinterpreted_batch_ndims=3) (image_networks.py:55-71; distributions/quantized.py:50-204)."""

  def __init__(self, h: torch.Tensor):
    Cc = h.shape[-1] // 2
    self.loc = 127.5 * (h[..., :Cc] + 1.0)                                      # pixel units
    self.scale = (torch.nn.functional.softplus(h[..., Cc:]) + math.exp(-7.0)) * 127.5

  event_shape = property(lambda self: tuple(self.loc.shape[1:]))
  batch_shape = property(lambda self: (self.loc.shape[0],))

  def mean(self):
    return self.loc / 255.0      # quantized.py:185-187 (`_pixels_to`, sigmoid domain)

  def stddev(self):
    return self.scale * (math.pi / math.sqrt(3.0))

  def _logcdf(self, j):
    r = -torch.nn.functional.softplus(-(j + 0.5 - self.loc) / self.scale)
    r = torch.where(j < 0.0, torch.full_like(r, -float('inf')), r)
    return torch.where(j < 255.0, r, torch.zeros_like(r))

  def _logsf(self, j):
    r = -torch.nn.functional.softplus((j + 0.5 - self.loc) / self.scale)
    r = torch.where(j < 0.0, torch.zeros_like(r), r)
    return torch.where(j < 255.0, r, torch.full_like(r, -float('inf')))

  def log_prob(self, x):
    e = self.log_prob_elem(x)
    return e.reshape(e.shape[0], -1).sum(1)

  def log_prob_elem(self, x):
    y = x * 255.0
    lsy, lsy1 = self._logsf(torch.ceil(y)), self._logsf(torch.ceil(y - 1.0))
    lcy, lcy1 = self._logcdf(torch.floor(y)), self._logcdf(torch.floor(y - 1.0))
    use_sf = lsy < lcy
    big, small = torch.where(use_sf, lsy1, lcy), torch.where(use_sf, lsy, lcy1)
    fin = torch.isfinite(small)
    d = torch.where(fin, big - small, torch.ones_like(big))
    l1m = torch.where(d < math.log(2.0), torch.log(-torch.expm1(-d)), torch.log1p(-torch.exp(-d)))
    return big + torch.where(fin, l1m, torch.zeros_like(l1m))

  def sample(self, n=None):
    shp = tuple(self.loc.shape) if n is None else (int(n),) + tuple(self.loc.shape)
    u = torch.rand(shp, device=self.loc.device).clamp_(1e-6, 1 - 1e-6)
    xs = self.loc + self.scale * (torch.log(u) - torch.log1p(-u)) - 0.5  # Logistic shifted by -1/2
    return torch.ceil(xs).clamp_(0.0, 255.0) / 255.0


class MixtureQuantizedLogisticObservation:
  """MixtureQuantizedLogistic(params, n_components=10, n_channels=C, low=0, high=255,
  inputs_domain='sigmoid') (distributions/quantized.py:206-381; image_networks.py:72-85): the
  decoder's K * (1 + 2C + C(C-1)/2) maps are (mixture logit | loc | raw scale | channel coefficients)
  per component."""

  def __init__(self, h: torch.Tensor, n_channels: int, n_components: int = 10):
    C, K = int(n_channels), int(n_components)
    no = 2 * C + C * (C - 1) // 2 + 1
    assert h.shape[-1] == K * no, (h.shape, K, no)
    hh = h.reshape(tuple(h.shape[:-1]) + (K, no))
    self.C, self.K = C, K
    self.logits, self.locs = hh[..., 0], hh[..., 1:1 + C]
    self.scales = torch.nn.functional.softplus(hh[..., 1 + C:1 + 2 * C]) + math.exp(-7.0)
    self.coefs = hh[..., 1 + 2 * C:]
    self._shape = tuple(h.shape[1:-1]) + (C,)

  event_shape = property(lambda self: self._shape)
  batch_shape = property(lambda self: (self.logits.shape[0],))

  def _chain(self, base):
    """loc_i += sum_{j<i} base_j * coef (quantized.py:315-320 with the transformed pixel values,
    :360-364 with the component means)."""
    cols = [self.locs[..., i] for i in range(self.C)]
    cnt = 0
    for i in range(self.C):
      for j in range(i):
        cols[i] = cols[i] + (base[..., None, j] if base is not None else cols[j]) * self.coefs[..., cnt]
        cnt += 1
    return torch.stack(cols, -1)

  def mean(self):
    m = 127.5 * (self._chain(None) + 1.0) - 0.5     # Shift(-0.5) of the base logistic (:373-375)
    pi = torch.softmax(self.logits, -1)
    return (pi[..., None] * m).sum(-2) / 255.0      # `_pixels_to`, sigmoid domain

  def log_prob(self, x):
    le = self._chain(2.0 * x - 1.0)
    comp = QuantizedLogisticObservation.__new__(QuantizedLogisticObservation)
    comp.loc, comp.scale = 127.5 * (le + 1.0), self.scales * 127.5
    xb = x[..., None, :].expand(le.shape)
    B = x.shape[0]
    # per (pixel, component, channel) terms, then the mixture over components, then the pixels
    q = comp.log_prob_elem(xb)
    pix = torch.logsumexp(torch.log_softmax(self.logits, -1) + q.sum(-1), -1)
    return pix.reshape(B, -1).sum(1)

  def sample(self, n=None):
    """The reference leaves sampling as a TODO that returns uniform noise of the image shape
    (quantized.py:383-386); restated as such."""
    shp = (self.logits.shape[0],) + self._shape
    if n is not None:
      shp = (int(n),) + shp
    return torch.rand(shp, device=self.logits.device)


# ======================================================================================
# training step objects
# ======================================================================================
@dataclass
class TrainStep:
  """odin/networks/base_networks.py:130-173"""
  inputs: Any = None
  training: bool = True
  mask: Any = None
  parameters: Any = None
  optimizer: Any = None
  name: str = ''

  def call(self):
    raise NotImplementedError

  def __call__(self):
    return self.call()


@dataclass
class VAEStep(TrainStep):
  """variational_autoencoder.py:111-126: loss = -mean(elbo(llk, kl)); metrics = means."""
  vae: 'VariationalAutoencoder' = None
  call_kw: Dict[str, Any] = field(default_factory=dict)

  def call(self):
    llk, kl = self.vae.elbo_components(self.inputs, training=self.training, mask=self.mask,
                                       **self.call_kw)
    loss = -torch.mean(self.vae.elbo(llk, kl))
    metrics = {k: torch.mean(v) for k, v in llk.items()}
    metrics.update({k: torch.mean(v) if torch.is_tensor(v) else v for k, v in kl.items()})
    return loss, metrics


# ======================================================================================
# the model
# ======================================================================================
def _as_tensor(x, device):
  if torch.is_tensor(x):
    return x.to(device=device, dtype=torch.float32).contiguous()
  return torch.as_tensor(np.asarray(x), dtype=torch.float32, device=device).contiguous()


class VariationalAutoencoder:
  """See module docstring.  Construction mirrors
  ``vae_cls(**get_networks(ds_name))`` of the reference (examples/vae/utils.py:231-256)."""

  def __init__(self, observation: RVconf = None, latents: RVconf = None,
               encoder: SequentialNetwork = None, decoder: SequentialNetwork = None,
               analytic: bool = False, reverse: bool = True, free_bits: Optional[float] = None,
               sample_shape=(), allow_negative_kl: bool = True, path: Optional[str] = None,
               step: int = 0, name: str = 'VariationalAutoencoder', device=None, seed: int = 1,
               lib=None, **kwargs):
    if encoder is None or decoder is None or latents is None or observation is None:
      d = get_networks('dense')
      encoder = encoder or d['encoder']
      decoder = decoder or d['decoder']
      latents = latents or d['latents']
      observation = observation or d['observation']
    for n, net in (('encoder', encoder), ('decoder', decoder)):
      if not isinstance(net, SequentialNetwork):
        raise ValueError(f'{n} must be a SequentialNetwork description, got {type(net)}')
    posterior = latents.posterior
    if posterior not in ('mvndiag', 'diag', 'normaldiag', 'mvntril', 'tril', 'relaxedonehot', 'relaxedsoftmax',
                         'relaxedbern', 'relaxedsigmoid', 'relaxedbernoulli'):
      raise ValueError(f"latents posterior {latents.posterior!r} is outside the HIP path "
                       f"(supported: 'mvndiag', 'mvntril', 'relaxedonehot', 'relaxedbernoulli')")
    self._latent_cov = 'tril' if posterior in ('mvntril', 'tril') else 'diag'
    self._latent_dist = 'relaxedonehot' if posterior in ('relaxedonehot', 'relaxedsoftmax') else 'normal'
    if posterior in ('relaxedbern', 'relaxedsigmoid', 'relaxedbernoulli'):
      self._latent_dist = 'relaxedbernoulli'
    # (the default temperature of RelaxedOneHotCategoricalLayer and RelaxedBernoulliLayer, discrete.py:286-343, 346 ff.)
    self._temperature = float(latents.kwargs.get('temperature', 0.5))
    if self._latent_dist == 'relaxedbernoulli':
      if self._relaxedbern_refusal is not None:
        raise ValueError(f"{type(self).__name__} with a 'relaxedbernoulli' posterior: {self._relaxedbern_refusal}")
      if len(tuple(latents.event_shape)) != 1:
        raise ValueError(f"'relaxedbernoulli': event_shape={latents.event_shape} must be one axis of binary units")
      if not self._temperature > 0.0:
        raise ValueError(f"'relaxedbernoulli': temperature={self._temperature} must be positive")
      if not reverse:
        raise NotImplementedError(RELAXEDBERN_NO_FORWARD_KL)
    if self._latent_dist == 'relaxedonehot':
      if self._concrete_refusal is not None:
        raise ValueError(f"{type(self).__name__} with a 'relaxedonehot' posterior: {self._concrete_refusal}")
      if len(tuple(latents.event_shape)) != 1:
        raise ValueError(f"'relaxedonehot': event_shape={latents.event_shape} must be one K-way variable")
      if not self._temperature > 0.0:
        raise ValueError(f"'relaxedonehot': temperature={self._temperature} must be positive")
      if not reverse:
        raise NotImplementedError(CONCRETE_NO_FORWARD_KL)
    if self._latent_cov == 'tril':
      if self._tril_refusal is not None:
        raise ValueError(f"{type(self).__name__} with a 'mvntril' posterior: {self._tril_refusal}")
      if not reverse:
        raise NotImplementedError("'mvntril' with reverse=False: KL(p || q) needs the inverse of L")
    sample_shape = (sample_shape,) if isinstance(sample_shape, int) else tuple(sample_shape)
    if len(sample_shape) > 1:
      raise ValueError(f'sample_shape={sample_shape}: at most one sample axis')
    if not reverse and not analytic:
      raise TypeError('reverse=False needs analytic=True (the reference cannot evaluate the '
                      'Monte-Carlo form of KL(p||q) either, helpers.py:261-276)')
    self.observation, self.latents, self.encoder, self.decoder = observation, latents, encoder, decoder
    self.analytic, self.reverse, self.free_bits = bool(analytic), bool(reverse), free_bits
    self.sample_shape, self.allow_negative_kl = tuple(sample_shape), allow_negative_kl
    self.path, self.name = path, name
    self._step = int(step)
    self.seed = int(seed)
    self.device = torch.device(device if device is not None else
                               ('cuda' if torch.cuda.is_available() else 'cpu'))
    self._lib = lib
    self._engines: Dict[int, VAEEngine] = {}
    self._params: Optional[torch.Tensor] = None
    self._optim_state = None
    self._last_outputs = None
    self._tc_mode = None
    self._capacity_mode = False
    self.trainer = None
    self.input_shape = tuple(encoder.input_shape) if encoder.input_shape else None
    self.zdim = int(latents.event_size)
    if self.input_shape is not None:
      self.build((None,) + self.input_shape)

  # ------------------------------------------------------------------ construction
  def build(self, input_shape):
    shape = tuple(input_shape)[1:]
    self.input_shape = shape
    eng = self._engine(1)  # validates shapes, allocates + initialises parameters
    return self

  def input_buffer(self, batch_size: int) -> torch.Tensor:
    """The float32 [B, H, W, C] tensor the captured training-step graph for this batch size
    reads: hand it to `odin_ai_amd.data.DeviceImageDataset(out=...)` (or fill it in place) and
    pass the batches it yields to `fit` / `optimize` -- no per-step input copy."""
    return self._engine(int(batch_size)).input_buffer()

  def _engine(self, B: int) -> VAEEngine:
    if self.input_shape is None:
      raise RuntimeError('model is not built: call build((None, H, W, C)) first')
    if B not in self._engines:
      eng = VAEEngine(self.encoder.layers, self.decoder.layers, self.input_shape, self.zdim, B,
                      self.device, observation=self.observation.posterior,
                      analytic=self.analytic, reverse=self.reverse, free_bits=self.free_bits,
                      tc=self._tc_mode, capacity=self._capacity_mode,
                      lib=self._lib, params=self._params, seed=self.seed + self._rank(),
                      optim_state=self._optim_state, world_size=self._world_size(),
                      force_dp=bool(getattr(self, 'force_dp', False)), latent_cov=self._latent_cov,
                      **self._latent_dist_options(),
                      **self._reg_options(), **getattr(self, 'engine_options', {}))
      if self._params is None:
        self._params = eng.params
        self._optim_state = (eng.m, eng.v)
        self._init_parameters(eng)
        # data parallel: every replica starts from rank 0's weights; the noise streams differ
        # per rank (seed + rank above), the weights must not
        from .dist import broadcast_parameters
        broadcast_parameters(eng.params, src=0)
      self._engines[B] = eng
    return self._engines[B]

  def _latent_dist_options(self) -> dict:
    """the engine keywords of a non-Gaussian posterior (none for the Gaussian ones: their engines are built with the
    arguments they always were)"""
    if self._latent_dist == 'normal':
      return {}
    return dict(latent_dist=self._latent_dist, temperature=self._temperature)

  def _world_size(self) -> int:
    import torch.distributed as dist
    return dist.get_world_size() if (dist.is_available() and dist.is_initialized()) else 1

  def _rank(self) -> int:
    import torch.distributed as dist
    return dist.get_rank() if (dist.is_available() and dist.is_initialized()) else 0

  def _init_parameters(self, eng: VAEEngine):
    """HeNormal for elu convs, glorot_uniform for Dense, glorot_normal for the latent
    projection, zero biases (image_networks.py:157-174; dense_distribution.py:124)."""
    g = torch.Generator(device='cpu').manual_seed(self.seed)
    deconv = {r.key for r in eng.enc_recs + eng.dec_recs if r.kind == 'deconv'}
    for key, shp, off in eng.layout.entries:
      n = int(np.prod(shp))
      if key[0] in ('vamp', 'vq'):   # (drawn by the engine: VAEEngine._init_pseudoinputs / init_codebook)
        continue
      if key[-1] == 'b':
        eng.params[off:off + n].zero_()
        continue
      if len(shp) == 4:
        fan_in = shp[0] * shp[1] * (shp[3] if key[:2] in deconv else shp[2])
        w = torch.nn.init.trunc_normal_(torch.empty(n), 0.0, 1.0, -2.0, 2.0, generator=g)
        w = w * math.sqrt(2.0 / fan_in) / 0.87962566
      elif key[0] == 'lat':
        w = torch.randn(n, generator=g) * math.sqrt(2.0 / (shp[0] + shp[1]))
      else:
        lim = math.sqrt(6.0 / (shp[0] + shp[1]))
        w = (torch.rand(n, generator=g) * 2 - 1) * lim
      eng.params[off:off + n] = w.to(self.device)

  # ------------------------------------------------------------------ properties
  @property
  def step(self) -> int:
    return self._step

  @property
  def n_parameters(self) -> int:
    return self._engine(1).n_params

  @property
  def last_outputs(self):
    return self._last_outputs

  @property
  def trainable_variables(self) -> Dict[tuple, torch.Tensor]:
    return self._engine(1).param_views()

  def set_elbo_configs(self, analytic=None, reverse=None, free_bits=None, sample_shape=None):
    """odin/bay/vi/_base.py:51-89"""
    if reverse is not None and not reverse and self._latent_cov == 'tril':
      raise NotImplementedError("'mvntril' with reverse=False: KL(p || q) needs the inverse of L")
    if reverse is not None and not reverse and self._latent_dist == 'relaxedonehot':
      raise NotImplementedError(CONCRETE_NO_FORWARD_KL)
    if reverse is not None and not reverse and self._latent_dist == 'relaxedbernoulli':
      raise NotImplementedError(RELAXEDBERN_NO_FORWARD_KL)
    if analytic is not None:
      self.analytic = bool(analytic)
    if reverse is not None:
      self.reverse = bool(reverse)
    if free_bits is not None:
      self.free_bits = free_bits
    if sample_shape is not None:
      self.sample_shape = (sample_shape,) if isinstance(sample_shape, int) else tuple(sample_shape)
    for e in self._engines.values():
      e.set_kl_form(self.analytic, self.reverse)
      e.free_bits = -1.0 if self.free_bits is None else float(self.free_bits)
    return self

  @property
  def n_samples(self) -> int:
    """prod(sample_shape): MC samples of z per input (variational_autoencoder.py:288-314)."""
    n = 1
    for i in self.sample_shape:
      n *= int(i)
    return n

  def _tile(self, x: torch.Tensor) -> torch.Tensor:
    """sample_shape = (n,): the reference draws z of shape [n, B, D] from one encoder pass and
    decodes n*B codes; llk / kl come out as [n, B] and the loss is their overall mean.  Here
    the batch is tiled n times (each copy gets its own noise): the same [n, B] values and the
    same gradients, at the price of n encoder passes."""
    n = self.n_samples
    return x if n == 1 else x.repeat((n,) + (1,) * (x.dim() - 1))

  @property
  def beta(self) -> float:
    return 1.0

  def _hyper_extra(self) -> dict:
    """per-step scalars beyond (lr, beta) that a subclass hands to the engine (BetaCapacityVAE: the capacity)"""
    return {}

  def _prior_log_prob(self, eng: VAEEngine, z: torch.Tensor, lp: torch.Tensor):
    """marginal_log_prob: lp [n, B] holds log N(z; 0, I) of the samples z [n, B, D]; a model with another prior
    overwrites it (VampriorVAE)"""

  def _step_metrics(self, out: torch.Tensor, metrics: Dict[str, torch.Tensor]):
    """optimize: a subclass's view of the step scalars out = [loss, mean llk, mean beta * kl, extra term]"""

  # the batch regulariser of InfoVAE / DIPVAE: engine options and the key of its term in `kl` / the metrics
  _reg_key: Optional[str] = None

  def _reg_options(self) -> dict:
    return {}

  # why a model class cannot take the full-covariance posterior ('mvntril'); None: it can
  _tril_refusal: Optional[str] = None
  # the same for the relaxed one-hot posterior ('relaxedonehot')
  _concrete_refusal: Optional[str] = None
  # and for the relaxed Bernoulli posterior ('relaxedbernoulli')
  _relaxedbern_refusal: Optional[str] = None

  # ------------------------------------------------------------------ forward API
  def _posterior(self, eng: VAEEngine) -> Union[MVNDiagPosterior, MVNTriLPosterior, RelaxedOneHotPosterior,
                                                RelaxedBernoulliPosterior]:
    if self._latent_dist == 'relaxedonehot':
      return RelaxedOneHotPosterior(eng.p.clone(), eng.z.clone(), eng.eps.clone(), self._temperature)
    if self._latent_dist == 'relaxedbernoulli':
      return RelaxedBernoulliPosterior(eng.p.clone(), eng.z.clone(), eng.eps.clone(), self._temperature)
    cls = MVNTriLPosterior if self._latent_cov == 'tril' else MVNDiagPosterior
    return cls(eng.p.clone(), eng.z.clone(), eng.D)

  def _observation_dist(self, h: torch.Tensor):
    if self.observation.posterior == 'bernoulli':
      return BernoulliObservation(h)
    if self.observation.posterior == 'cbernoulli':
      return ContinuousBernoulliObservation(h)
    if self.observation.posterior == 'nb':
      return NegativeBinomialObservation(h, self._lib)
    if self.observation.posterior == 'zinb':
      return ZINegativeBinomialObservation(h, self._lib)
    if self.observation.posterior == 'qlogistic':
      return QuantizedLogisticObservation(h)
    if self.observation.posterior == 'mixqlogistic':
      return MixtureQuantizedLogisticObservation(h, self.input_shape[-1],
                                                 self.observation.kwargs.get('n_components', 10))
    return GaussianObservation(h, self.observation.posterior == 'gaussian_softplus1')

  def encode(self, inputs, training=None, mask=None, only_encoding=False, eps=None, **kwargs):
    """variational_autoencoder.py:288-314"""
    x = _as_tensor(inputs, self.device)
    eng = self._engine(x.shape[0])
    eng.set_hyper(beta=self.beta, t=self._step, **self._hyper_extra())
    eng.run_encoder(x, None if eps is None else _as_tensor(eps, self.device))
    if only_encoding:
      return eng.enc.outs[-1].clone()
    return self._posterior(eng)

  def decode(self, latents, training=None, mask=None, only_decoding=False, **kwargs):
    """variational_autoencoder.py:316-360"""
    z = latents.tensor() if isinstance(latents, (MVNDiagPosterior, MVNTriLPosterior, RelaxedOneHotPosterior,
                                                 RelaxedBernoulliPosterior)) else latents
    z = _as_tensor(z, self.device)
    eng = self._engine(z.shape[0])
    h = eng.run_decoder(z).clone()
    return h if only_decoding else self._observation_dist(h)

  def call(self, inputs, training=None, mask=None, eps=None, **kwargs):
    """variational_autoencoder.py:362-394 -> (p(x|z), q(z|x))"""
    qz_x = self.encode(inputs, training=training, mask=mask, eps=eps)
    px_z = self.decode(qz_x, training=training, mask=mask)
    self._last_outputs = (px_z, qz_x)
    return px_z, qz_x

  __call__ = call

  def elbo_components(self, inputs, training=None, mask=None, eps=None, **kwargs):
    """variational_autoencoder.py:515-542.  One fused engine pass: llk [B], kl [B]
    (already multiplied by beta for the Beta family, beta_vae.py:38-43)."""
    x = self._tile(_as_tensor(inputs, self.device))
    n = self.n_samples
    eng = self._engine(x.shape[0])
    eng.set_hyper(beta=self.beta, t=self._step, **self._hyper_extra())
    eng.forward(x, None if eps is None else _as_tensor(eps, self.device).reshape(x.shape[0], -1))
    qz_x = self._posterior(eng)
    px_z = self._observation_dist(eng.dec.outs[-1].clone())
    self._last_outputs = (px_z, qz_x)
    shp = (lambda t: t.reshape(n, -1)) if n > 1 else (lambda t: t)
    llk = {f'llk_{self.observation.name}': shp(eng.llk.clone())}
    klv = shp(eng.kl.clone() * self.beta)
    if self.analytic:
      klv = klv[:1] if n > 1 else klv.unsqueeze(0)  # [1, B] (helpers.py:370-371)
    kl = {f'kl_{self.latents.name}': klv}
    if self._tc_mode == 'betatc':
      kl[f'tc_{self.latents.name}'] = (self.beta - 1.0) * eng.tc_ws[0].clone()
    if self._reg_key is not None:   # reg_coef * value, the term the loss carries (NOT multiplied by beta)
      kl[f'{self._reg_key}_{self.latents.name}'] = eng.out4[3].clone()
    return llk, kl

  def elbo(self, llk: Dict[str, torch.Tensor], kl: Dict[str, torch.Tensor]) -> torch.Tensor:
    """odin/bay/vi/_base.py:151-194: sum(llk) - sum(kl), broadcasting scalars / [1,B]."""
    L = 0.0
    for v in llk.values():
      L = L + v
    K = 0.0
    for k, v in kl.items():
      if not self.allow_negative_kl and torch.is_tensor(v):
        if bool((v < -1e-3).any()):
          raise AssertionError(f'negative KL for {k}')
      K = K + v
    return L - K

  def sample_prior(self, n: int = 1, seed: int = 1) -> torch.Tensor:
    g = torch.Generator(device='cpu').manual_seed(int(seed))
    if self._latent_dist == 'relaxedonehot':   # OneHotCategorical with equal logits: one-hot rows
      idx = torch.randint(self.zdim, (int(n),), generator=g)
      return torch.nn.functional.one_hot(idx, self.zdim).to(dtype=torch.float32, device=self.device)
    if self._latent_dist == 'relaxedbernoulli':   # Independent(Bernoulli(logits=0)): 0 / 1 entries of probability 1/2
      return torch.randint(2, (int(n), self.zdim), generator=g).to(dtype=torch.float32, device=self.device)
    return torch.randn(int(n), self.zdim, generator=g).to(self.device)

  def sample_observation(self, n: int = 1, seed: int = 1, training=False, **kwargs):
    return self.decode(self.sample_prior(n, seed=seed), training=training)

  def marginal_log_prob(self, inputs, training=None, n_mcmc: Optional[int] = 100,
                        reduce: Optional[Callable] = torch.mean, batch_size: int = 32,
                        verbose: bool = False, eps=None, **kwargs):
    """variational_autoencoder.py:396-513: per batch ONE encoder pass, n_mcmc posterior samples
    per input, one decoder pass over the n_mcmc*B codes, log-mean-exp over the samples on
    device.  Returns the reference's structure: ({name: llk}, {name: (log q, log p)}) with
    llk = logsumexp_k log p(x|z_k) - log n and the same log-mean-exp of log q(z_k|x), log p(z_k);
    `reduce` (default mean over inputs) is applied to each, None keeps the per-input vectors.
    `eps` ([n_mcmc, N, D], optional) fixes the noise for parity tests."""
    x_all = _as_tensor(inputs, self.device)
    n = int(n_mcmc) if n_mcmc is not None else self.n_samples
    N, D = x_all.shape[0], self.zdim
    outs = {'llk': [], 'lq': [], 'lp': []}
    f32 = dict(dtype=torch.float32, device=self.device)
    for i0 in range(0, N, int(batch_size)):
      x = x_all[i0:i0 + int(batch_size)].contiguous()
      B = x.shape[0]
      eng = self._engine(B)
      lib, st = eng.lib, eng.stream()
      eng.set_hyper(beta=1.0, t=self._step, **self._hyper_extra())
      eng.run_encoder(x)  # fills eng.p = (loc | raw scale)
      concrete = self._latent_dist == 'relaxedonehot'
      relaxedbern = self._latent_dist == 'relaxedbernoulli'
      if eps is None:
        e = torch.empty(n, B, D, **f32)
        rng = lib.odin_rng_gumbel if concrete else lib.odin_rng_logistic if relaxedbern else lib.odin_rng_normal
        rng(e.data_ptr(), n * B * D, self.seed + 7919 + i0, eng.hp(N_HYPER), st)
      else:
        e = _as_tensor(eps, self.device)[:, i0:i0 + B].contiguous()
      z = torch.empty(n, B, D, **f32)
      lq, lp, llk = torch.empty(n, B, **f32), torch.empty(n, B, **f32), torch.empty(n, B, **f32)
      if concrete:
        lib.odin_latent_concrete_sample_logprob(eng.p.data_ptr(), e.data_ptr(), z.data_ptr(), lq.data_ptr(),
                                                lp.data_ptr(), n, B, D, self._temperature, st)
      elif relaxedbern:
        lib.odin_latent_relaxedbern_sample_logprob(eng.p.data_ptr(), e.data_ptr(), z.data_ptr(), lq.data_ptr(),
                                                   lp.data_ptr(), n, B, D, self._temperature, st)
      else:
        sample_logprob = (lib.odin_latent_tril_sample_logprob if self._latent_cov == 'tril'
                          else lib.odin_latent_sample_logprob)
        sample_logprob(eng.p.data_ptr(), e.data_ptr(), z.data_ptr(), lq.data_ptr(), lp.data_ptr(), n, B, D, st)
      self._prior_log_prob(eng, z, lp)
      # decode the n*B codes in chunks of whole sample-rows (bounded activation memory)
      rows = max(1, min(n, 2048 // max(B, 1)))
      for k0 in range(0, n, rows):
        r = min(rows, n - k0)
        de = self._engine(r * B)
        de.set_hyper(beta=1.0, t=self._step, **self._hyper_extra())
        h = de.run_decoder(z[k0:k0 + r].reshape(r * B, D))
        xt = x.repeat((r,) + (1,) * (x.dim() - 1))
        de.observation_llk(h, xt, llk[k0:k0 + r].reshape(r * B))
      for key, src in (('llk', llk), ('lq', lq), ('lp', lp)):
        o = torch.empty(B, **f32)
        lib.odin_logmeanexp_rows(src.data_ptr(), o.data_ptr(), n, B, st)
        outs[key].append(o)
    cat = {k: torch.cat(v) for k, v in outs.items()}
    if reduce is not None:
      cat = {k: reduce(v) for k, v in cat.items()}
    return ({self.observation.name: cat['llk']},
            {self.latents.name: (cat['lq'], cat['lp'])})

  # ------------------------------------------------------------------ training
  def train_steps(self, inputs, training=None, mask=None, name: str = '', **kwargs
                  ) -> Iterator[VAEStep]:
    """variational_autoencoder.py:545-558"""
    yield VAEStep(vae=self, parameters=self.trainable_variables, inputs=inputs,
                  training=training, mask=mask, name=name, call_kw=kwargs)

  def _lr(self, learning_rate) -> float:
    return float(learning_rate(self._step)) if callable(learning_rate) else float(learning_rate)

  def optimize(self, inputs, training: bool = True, optimizer=None, learning_rate=1e-4,
               clipnorm=None, clipvalue=None, global_clipnorm=None, skip_update_threshold=None,
               when_skip_update: int = 0, nan_gradients_policy: str = 'skip',
               allow_none_gradients=False, aggregate_gradients=False, track_gradients=False,
               eps=None, use_graph: bool = False):
    """Networks.optimize (base_networks.py:415-624): step += 1; forward; backward; NaN policy;
    skip_update_threshold -> per-variable clipnorm -> clip_by_global_norm -> clipvalue (the
    reference's order, :549-596); Adam.  Returns (loss, metrics) as device scalars.

    nan_gradients_policy: 'ignore' applies the update whatever the gradients hold; every other
    policy leaves parameters and optimiser state untouched on device when a gradient is not
    finite and raises `nan_flag` (polled by `fit`, which stops / raises / restores the last
    checkpoint).  (The reference zeroes the gradients with `g - g`, which is NaN again for a NaN
    gradient, and hands them to Adam: a step it cannot survive.  Not reproduced.)
    aggregate_gradients only matters for multi-step models (FactorVAE); track_gradients adds the
    gradient tensors as `_grad/<variable>` metrics (:609-611)."""
    if nan_gradients_policy not in ('stop', 'skip', 'raise', 'ignore', 'restore'):
      raise ValueError(f'nan_gradients_policy={nan_gradients_policy!r}')
    x = self._tile(_as_tensor(inputs, self.device))
    eng = self._engine(x.shape[0])
    if eps is not None:
      eps = _as_tensor(eps, self.device).reshape(x.shape[0], -1)
    if training:
      self._step += 1
    eng.step_count = self._step - 1 if training else self._step
    if not training:
      eng.set_hyper(beta=self.beta, t=self._step, **self._hyper_extra())
      eng.forward(x, eps)
    else:
      eng.train_step(x, eps,
                     lr=self._lr(learning_rate), beta=self.beta,
                     global_clipnorm=global_clipnorm, use_graph=use_graph, clipnorm=clipnorm,
                     clipvalue=clipvalue, skip_update_threshold=skip_update_threshold,
                     when_skip_update=when_skip_update,
                     check_nan=nan_gradients_policy != 'ignore', **self._hyper_extra())
      self._step = eng.step_count
    out = eng.out4.clone()
    metrics = {f'llk_{self.observation.name}': out[1], f'kl_{self.latents.name}': out[2]}
    if self._tc_mode == 'betatc':
      metrics[f'tc_{self.latents.name}'] = out[3]
    if self._reg_key is not None:
      metrics[f'{self._reg_key}_{self.latents.name}'] = out[3]
    self._step_metrics(out, metrics)
    if training and track_gradients:
      for k, g in eng.grad_views().items():
        metrics['_grad/' + self.variable_name(k)] = g.clone()
    return out[0], metrics

  def _fit_batch(self, b):
    """one element of an iterable `train` / `valid` of fit as what optimize takes (MultitaskVAE: also 3-tuples)"""
    return _as_tensor(b, self.device)

  def _fit_batch_rows(self, xb) -> int:
    """the batch size of the engine that ran such an element"""
    return xb.shape[0]

  @property
  def nan_flag(self) -> bool:
    """True when a training step met non-finite gradients and skipped its update (host sync)."""
    return any(int(e.flag.item()) != 0 for e in self._engines.values())

  def _nan_flags(self, eng: VAEEngine) -> List[torch.Tensor]:
    """the device flags `fit` polls for the step it just ran (TwoStageVAE: the second optimiser's in stage 2)"""
    return [eng.flag]

  @property
  def skipped_update(self) -> int:
    """Networks.skipped_update (base_networks.py:573-577): updates zeroed by skip_update_threshold."""
    return sum(int(e.skipped_update.item()) for e in self._engines.values())

  def variable_name(self, key: tuple) -> str:
    """Keras variable name of a parameter key: the reference's layer names
    (image_networks.py:248-268,463-511: encoder0.., encoder_proj, decoder_proj, decoder1..;
    DistributionDense 'latents', dense_distribution.py:229-238) + /kernel | /bias."""
    if key[0] == 'vamp':
      return VAMPRIOR_VARIABLE
    if key[0] == 'vq':
      return f'{VQ_LAYER}/{key[1]}'
    suffix = 'kernel' if key[-1] == 'w' else 'bias'
    if key[0] == 'lat':
      return f'{self.latents.name}/{suffix}'
    net = self.encoder if key[0] == 'enc' else self.decoder
    names = layer_names(net, 'encoder' if key[0] == 'enc' else 'decoder')
    return f'{names[key[1]]}/{suffix}'

  def fit(self, train, *, valid=None, valid_freq: int = 500, valid_interval: float = 0,
          optimizer='adam', learning_rate=1e-4, clipnorm=None, global_clipnorm=None,
          clipvalue=None, skip_update_threshold=None, when_skip_update=None, epochs: int = -1,
          max_iter: int = 1000, batch_size: int = 32, on_batch_end=None, on_valid_end=None,
          compile_graph: bool = True, autograph: bool = False, logging_interval: float = 5,
          skip_fitted: Union[bool, int] = False, nan_gradients_policy: str = 'stop',
          logdir=None, allow_none_gradients=False, track_gradients=False, seed: int = 1,
          nan_check_interval: int = 50):
    """Networks.fit (base_networks.py:642-812) with Trainer.fit's cadence (training/trainer.py:536-738).
    `train` / `valid`: array / tensor [N,H,W,C] or an iterable of batches.  compile_graph -> the step is
    replayed as one HIP graph.  Validation (mean loss / metrics of the training=False step over `valid`,
    `last_valid_loss`, `last_valid_metrics`, `valid/*` scalars) and the `on_valid_end` callback run at the first
    iteration, whenever step % valid_freq == 0 and `valid_interval` seconds have passed (`valid_interval` > 0
    makes valid_freq 1), and once more when training ends; `on_batch_end` after every step; `train/*` scalars
    at most every `logging_interval` seconds (metrics whose name starts with '_' stay hidden)."""
    if optimizer not in ('adam', None) and not callable(optimizer):
      raise RuntimeError(f'No support for optimizer {optimizer!r} on the HIP path (adam only)')
    if nan_gradients_policy not in ('stop', 'skip', 'raise', 'ignore', 'restore'):
      raise ValueError(nan_gradients_policy)
    if skip_fitted and self._step >= (max_iter if skip_fitted is True else int(skip_fitted)):
      return self
    history = []

    def batches():
      if torch.is_tensor(train) or isinstance(train, np.ndarray):
        data = _as_tensor(train, self.device).contiguous()
        N = data.shape[0]
        g = torch.Generator(device='cpu').manual_seed(seed)
        ep = 0
        n_per = int(np.prod(data.shape[1:]))
        # the shuffled batch is gathered by ONE launch straight into the tensor the step graph reads (no torch
        # advanced-indexing kernel, no per-step copy into the static buffer)
        direct = (data.dtype == torch.float32 and n_per % 4 == 0 and tuple(data.shape[1:]) == tuple(self.input_shape)
                  and N >= batch_size)
        if direct:
          eng0 = self._engine(int(batch_size))
          xb0 = eng0.input_buffer()
        while epochs < 0 or ep < epochs:
          perm = torch.randperm(N, generator=g).to(device=self.device, dtype=torch.int32)
          for i in range(0, N - batch_size + 1, batch_size):
            if direct:
              eng0.lib.odin_gather_rows_f32(data.data_ptr(), perm.data_ptr() + 4 * i, xb0.data_ptr(),
                                            int(batch_size), n_per, eng0.stream())
              yield xb0
            else:
              yield data[perm[i:i + batch_size].long()].contiguous()
          ep += 1
      else:
        ep = 0
        while epochs < 0 or ep < epochs:
          for b in train:
            yield self._fit_batch(b)
          ep += 1

    # ---- validation / logging cadence of Trainer.fit (training/trainer.py:607-700): `valid_interval` > 0 takes
    # precedence over `valid_freq`; validation (and ALWAYS the on_valid_end callback) runs at the first
    # iteration, then whenever step % valid_freq == 0 and valid_interval seconds have passed, and once more
    # when training ends; train summaries are written at most every `logging_interval` seconds
    import time as _time
    valid_freq = max(1, int(valid_freq))
    valid_interval = float(valid_interval)
    if valid_interval > 0:
      valid_freq = 1

    def valid_batches():
      if torch.is_tensor(valid) or isinstance(valid, np.ndarray):
        data = _as_tensor(valid, self.device)
        N = data.shape[0]
        bs = min(batch_size, N)
        for i in range(0, N - bs + 1, bs):
          yield data[i:i + bs].contiguous()
      else:
        for b in valid:
          yield self._fit_batch(b)

    def run_valid():
      losses, mets = [], {}
      for vb in valid_batches():
        l, m = next(iter(self.train_steps(vb, training=False)))()
        losses.append(float(l))
        for k, v in m.items():
          mets.setdefault(k, []).append(float(v))
      if not losses:
        return None, {}
      return float(np.mean(losses)), {k: float(np.mean(v)) for k, v in mets.items()}

    def events(eng):
      if getattr(self, '_events', None) is None or self._events_dir != logdir:
        from .tf_checkpoint import ScalarEventWriter
        self._events, self._events_dir = ScalarEventWriter(logdir, lib=eng.lib), logdir
      return self._events

    def validate(eng):
      if valid is not None:
        vl, vm = run_valid()
        self.last_valid_loss, self.last_valid_metrics = vl, vm
        if vl is not None:
          self.valid_history.append((self._step, vl))
          if logdir is not None:
            ev = events(eng)
            ev.scalar('valid/loss', vl, self._step)
            for mk, mv in vm.items():
              if not mk.startswith('_'):
                ev.scalar(f'valid/{mk}', mv, self._step)
            ev.flush()
      if on_valid_end is not None:  # (the callback is always called, with or without a validation set)
        on_valid_end()

    self.valid_history = getattr(self, 'valid_history', [])
    self.last_valid_loss, self.last_valid_metrics = None, {}
    t_start = _time.monotonic()
    last_log, last_valid = -float('inf'), t_start
    it = 0
    eng = None
    for xb in batches():
      if it >= max_iter:
        break
      loss, metrics = self.optimize(xb, training=True, learning_rate=learning_rate,
                                    clipnorm=clipnorm, clipvalue=clipvalue,
                                    global_clipnorm=global_clipnorm,
                                    skip_update_threshold=skip_update_threshold,
                                    when_skip_update=when_skip_update or 0,
                                    nan_gradients_policy=nan_gradients_policy,
                                    track_gradients=track_gradients,
                                    use_graph=compile_graph and self.device.type == 'cuda')
      it += 1
      eng = self._engine(self._fit_batch_rows(xb))
      self.last_train_loss, self.last_train_metrics = loss, metrics
      if on_batch_end is not None:
        on_batch_end()
      now = _time.monotonic()
      # the NaN flag is sticky on device; polling it costs a host sync, so it is read every
      # `nan_check_interval` iterations (and at the end) unless the policy must act at once
      if it % nan_check_interval == 0 or it == max_iter:
        flags = self._nan_flags(eng)
        if any(int(f.item()) != 0 for f in flags):  # non-finite gradients: the update was skipped on device
          if nan_gradients_policy == 'raise':
            raise RuntimeError(f'NaNs gradient! (step {self._step})')
          if nan_gradients_policy == 'stop':
            break
          if nan_gradients_policy == 'restore':  # fall back to the last checkpoint (:543-545)
            self.load_weights(raise_notfound=False)
          for f in flags:
            f.zero_()
        history.append((self._step, float(loss)))
        # Trainer's TensorBoard scalars (training/trainer.py:52-71), at most every logging_interval seconds
        if logdir is not None and now - last_log >= float(logging_interval):
          ev = events(eng)
          ev.scalar('train/loss', float(loss), self._step)
          for mk, mv in metrics.items():
            if not mk.startswith('_'):   # (metrics hidden with a leading '_', trainer.py:662)
              ev.scalar(f'train/{mk}', float(mv), self._step)
          ev.flush()
          last_log = now
      if it == 1 or (self._step % valid_freq == 0 and now - last_valid >= valid_interval):
        validate(eng)
        last_valid = _time.monotonic()
    if eng is not None:
      validate(eng)  # final callback: training ended (trainer.py:704-709)
    self.history = history
    return self

  # ------------------------------------------------------------------ checkpoints
  def save_weights(self, filepath: Optional[str] = None, overwrite: bool = True,
                   save_format: str = 'tf'):
    """base_networks.py:373-390: weights + step (optimizer state deliberately not tracked).
    save_format='tf' (the reference's, :386): a TensorFlow checkpoint `<filepath>.index` +
    `<filepath>.data-00000-of-00001` whose object graph names every variable by its Keras name
    (`encoder0/kernel`, ..., `latents/bias`, `Step`) -- readable by `tf.train.load_checkpoint`;
    save_format='npz': one plain `.npz` with the same names.  No pickle either way."""
    filepath = filepath or self.path
    if filepath is None:
      raise ValueError('No path is given for saving weights')
    eng = self._engine(1)
    W = {self.variable_name(k): v.detach().cpu().numpy() for k, v in eng.param_views().items()}
    W.update(self._extra_checkpoint_variables())
    if save_format == 'tf':
      if os.path.exists(filepath + '.index') and not overwrite:
        raise RuntimeError(f'{filepath} exists')
      from . import tf_checkpoint
      W['Step'] = np.asarray(self._step, np.int64)   # base_networks.py:212
      tf_checkpoint.save_checkpoint(filepath, W, lib=eng.lib)
    elif save_format == 'npz':
      if os.path.exists(self._npz_path(filepath)) and not overwrite:
        raise RuntimeError(f'{filepath} exists')
      W['__step__'] = np.asarray(self._step, np.int64)
      with open(self._npz_path(filepath), 'wb') as f:
        np.savez(f, **W)
    else:
      raise ValueError(f"save_format={save_format!r} ('tf' | 'npz')")
    return self

  @staticmethod
  def _npz_path(filepath: str) -> str:
    return filepath if filepath.endswith('.npz') else filepath + '.npz'

  def load_weights(self, filepath: Optional[str] = None, raise_notfound: bool = False):
    """base_networks.py:338-371.  Reads a TensorFlow checkpoint (also one written by the
    reference: variables are found by their Keras names inside the checkpoint's object graph,
    whatever the object paths) or the `.npz` form."""
    filepath = filepath or self.path
    if filepath is not None and os.path.exists(filepath + '.index'):
      from . import tf_checkpoint
      d = tf_checkpoint.load_checkpoint(filepath, lib=self._engine(1).lib)
      step_keys = [k for k in d if k == 'Step' or k.endswith('/Step')]
      step = int(d[step_keys[0]]) if step_keys else self._step
    elif filepath is not None and os.path.exists(self._npz_path(filepath)):
      d = dict(np.load(self._npz_path(filepath), allow_pickle=False))
      step = int(d.pop('__step__'))
    else:
      if raise_notfound:
        raise FileNotFoundError(f'Cannot find saved weights at path: {filepath}')
      return self
    eng = self._engine(1)
    for k, v in eng.param_views().items():
      name = self.variable_name(k)
      a = self._find_variable(d, name)
      if tuple(a.shape) != tuple(v.shape):
        raise ValueError(f'{name}: checkpoint shape {a.shape} != {tuple(v.shape)}')
      v.copy_(torch.as_tensor(np.asarray(a), dtype=torch.float32, device=self.device))
    self._load_extra_checkpoint_variables(d)
    self._step = step
    return self

  def _extra_checkpoint_variables(self) -> Dict[str, np.ndarray]:
    """Variables beyond encoder / latents / decoder that Keras would track on this model
    (sub-layers and optimizers held as attributes): {checkpoint name: array}."""
    return {}

  def _load_extra_checkpoint_variables(self, d: Dict[str, np.ndarray]):
    pass

  @staticmethod
  def _find_variable(d: Dict[str, np.ndarray], name: str):
    """exact name first, then a unique '<prefix>/name' (a model nested in another)."""
    if name in d:
      return d[name]
    hits = [n for n in d if n.endswith('/' + name)]
    if len(hits) != 1:
      raise KeyError(f'{name}: {len(hits)} matching variables in the checkpoint ({hits[:3]})')
    return d[hits[0]]

  def __str__(self):
    return (f'{self.name}(input={self.input_shape}, zdim={self.zdim}, '
            f'params={self.n_parameters}, step={self._step}, device={self.device})')


# ======================================================================================
# Beta family
# ======================================================================================
class BetaVAE(VariationalAutoencoder):
  """beta_vae.py:11-43: every KL term multiplied by beta (constant or an Interpolation of
  the training step)."""

  def __init__(self, beta: Union[float, Interpolation] = 1.0, name='BetaVAE', **kwargs):
    self._beta = beta
    super().__init__(name=name, **kwargs)

  @property
  def beta(self) -> float:
    if isinstance(self._beta, Interpolation):
      return float(self._beta(self._step))
    return float(self._beta)

  @beta.setter
  def beta(self, b):
    self._beta = b


class BetaCapacityVAE(VariationalAutoencoder):
  """beta_vae.py:132-177 (Burgess et al. 2018, eq. 8): every KL term becomes gamma * |kl - C(step)| with the
  capacity C raised from c_min to c_max over n_steps by `interpolation` (backend/interpolation.py); `step` is the
  training step, incremented before the loss is evaluated (base_networks.py:478-479).  The latent kernels emit
  |kl - C| and its sign (odin_latent_fwd's `capacity` argument), so gamma takes the place beta has in BetaVAE."""

  def __init__(self, gamma: float = 10.0, c_min: float = 0.01, c_max: float = 25.0, n_steps: int = 10000,
               interpolation: str = 'linear', name='BetaCapacityVAE', **kwargs):
    from . import interpolation as interp
    self.gamma = float(gamma)
    self.interpolation = interp.get(str(interpolation))(vmin=float(c_min), vmax=float(c_max), steps=int(n_steps))
    super().__init__(name=name, **kwargs)
    self._capacity_mode = True
    self._engines.clear()

  @property
  def beta(self) -> float:  # the weight the engine multiplies the (capacity-shifted) KL by
    return self.gamma

  @property
  def capacity(self) -> float:
    return float(self.interpolation(self._step))

  def _hyper_extra(self) -> dict:
    return dict(capacity=self.capacity)


class AnnealingVAE(BetaVAE):
  """beta_vae.py:83-107: beta = linear(vmin=1e-6, vmax=1, steps=2000)(step)."""

  def __init__(self, vmin: float = 1e-6, vmax: float = 1.0, steps: int = 2000,
               name='AnnealingVAE', **kwargs):
    super().__init__(beta=linear(vmin=vmin, vmax=vmax, steps=steps), name=name, **kwargs)


class BetaTCVAE(BetaVAE):
  """beta_vae.py:110-129: + (beta-1) * total_correlation(z, q(z|x)) (losses.py:101-157);
  the KL is ALSO scaled by beta through BetaVAE.elbo_components (:42)."""

  _tril_refusal = 'the total-correlation estimator reads a diagonal scale'
  _concrete_refusal = 'the total-correlation estimator reads a Gaussian posterior'
  _relaxedbern_refusal = _concrete_refusal

  def __init__(self, beta: float = 1.0, name='BetaTCVAE', **kwargs):
    super().__init__(beta=beta, name=name, **kwargs)
    self._tc_mode = 'betatc'
    self._engines.clear()


class InfoVAE(BetaVAE):
  """info_vae.py:28-91: a BetaVAE with beta = 1 - alpha plus kl['div_<latents>'] = (lamda - beta) * MMD(q(z), p(z))
  (losses.py:222-276), added after BetaVAE scales the KL -- not multiplied by beta.  The MMD reuses the forward's
  sample (q_sample_shape=None) against p_sample_shape prior samples drawn on the device every step; its value and its
  gradient come from one launch per step (latent_reg.hip).  `divergence`: a functools.partial of
  maximum_mean_discrepancy; anything else the HIP path does not compute (another callable, q_sample_shape other than
  None, kernel='polynomial') raises NotImplementedError.  A `beta=` keyword is accepted and discarded, as the
  reference pops it."""

  def __init__(self, alpha: float = 0.0, lamda: float = 100.0,
               divergence: Callable = functools.partial(maximum_mean_discrepancy, kernel='gaussian',
                                                        q_sample_shape=None, p_sample_shape=100),
               name='InfoVAE', **kwargs):
    kwargs.pop('beta', None)
    if not callable(divergence):
      raise AssertionError(f'divergence must be callable, but given: {type(divergence)}')
    self.mmd_kernel, self.mmd_prior_samples = mmd_config(divergence)
    self.divergence = divergence
    self.lamda = float(lamda)
    super().__init__(beta=1.0 - float(alpha), name=name, **kwargs)

  @property
  def alpha(self) -> float:
    return 1.0 - self.beta

  @alpha.setter
  def alpha(self, alpha):
    self.beta = 1.0 - float(alpha)

  _reg_key = 'div'
  _concrete_refusal = "the MMD's prior sample is Gaussian"
  _relaxedbern_refusal = _concrete_refusal

  def _reg_options(self) -> dict:
    return dict(latent_reg='mmd', reg_coef=self.lamda - self.beta, mmd_kernel=self.mmd_kernel,
                mmd_prior_samples=self.mmd_prior_samples, prior_seed=self.seed)

  def _hyper_extra(self) -> dict:
    return dict(reg_coef=self.lamda - self.beta)


class DIPVAE(BetaVAE):
  """dip_vae.py: a BetaVAE plus kl['dip_<latents>'] = disentangled_inferred_prior_loss(q(z|x), only_mean,
  lambda_offdiag, lambda_diag) (losses.py:39-98), unscaled by beta; type I (only_mean) penalises Cov[E(z)], type II
  E[Cov(z)] + Cov[E(z)].  Value and gradient: one launch per step (latent_reg.hip)."""

  def __init__(self, only_mean: bool = False, lambda_diag: float = 1.0, lambda_offdiag: float = 2.0,
               beta: float = 1.0, name='DIPVAE', **kwargs):
    self.only_mean = bool(only_mean)
    self.lambda_diag, self.lambda_offdiag = float(lambda_diag), float(lambda_offdiag)
    super().__init__(beta=beta, name=name, **kwargs)

  _reg_key = 'dip'
  _tril_refusal = 'the disentangled-inferred-prior penalty reads a diagonal scale'
  _concrete_refusal = 'the disentangled-inferred-prior penalty reads a Gaussian mean and scale'
  _relaxedbern_refusal = _concrete_refusal

  def _reg_options(self) -> dict:
    return dict(latent_reg='dip_i' if self.only_mean else 'dip_ii', reg_coef=1.0,
                dip_lambda=(self.lambda_diag, self.lambda_offdiag))


# checkpoint name of the pseudo-input variable W_u [n_components, prod(input_shape)]: the kernel of the bias-free Dense
# layer `Vamprior.means` (vamprior.py:74-82).  Like the other names of the 'tf' format it has never been opened by
# TensorFlow itself.
VAMPRIOR_VARIABLE = 'vamprior/means/kernel'


class Vamprior:
  """vamprior.py:25-133: p(z) = 1/K sum_k q(z | u_k), the encoder's own posteriors at the K learned pseudo-inputs
  u = clip(W_u, 1e-6, 1 - 1e-6).  The components are recomputed from the model's current weights at every call."""

  def __init__(self, vae: 'VampriorVAE'):
    self._vae = vae
    self.n_components = int(vae.n_components)
    self.input_shape = tuple(vae.input_shape)

  def _eng(self) -> VAEEngine:
    """the model's batch-1 engine (always there: build() made it) with the components of the current weights"""
    eng = self._vae._engine(1)
    eng.pseudo_forward()
    return eng

  @property
  def pseudoinputs(self) -> torch.Tensor:
    """the clipped pseudo-inputs [K, *input_shape]"""
    return self._eng().vamp_u.clone()

  @property
  def distribution(self) -> MVNDiagPosterior:
    """q(z | u_k), k = 0 .. K - 1 (its cached sample: the means); ONE pass of the encoder at batch K -- take
    mean() / stddev() of the returned object when both are wanted"""
    eng = self._eng()
    p = eng.vamp_pu.clone()
    return MVNDiagPosterior(p, p[:, :eng.D].clone(), eng.D)

  def mean(self):
    return self.distribution.mean()

  def stddev(self):
    return self.distribution.stddev()

  def log_prob(self, z) -> torch.Tensor:
    """log p(z) [n] for z [n, D], any n: the mixture kernel, forward only (vamprior.hip), through the one engine"""
    z = _as_tensor(z, self._vae.device).reshape(-1, self._vae.zdim).contiguous()
    return self._eng().vamprior_log_prob(z, torch.empty(z.shape[0], dtype=torch.float32, device=z.device))

  def sample(self, n: int = 1, seed: Optional[int] = None) -> torch.Tensor:
    """_sample_n (vamprior.py:121-131): n DISTINCT components by a seeded shuffle, one posterior sample of each.
    (TensorFlow's random stream is not reproduced: the draw is a function of `seed` through torch's generator.)"""
    n = int(n)
    if not 1 <= n <= self.n_components:
      raise ValueError(f'Vamprior.sample: n={n} outside [1, n_components={self.n_components}] (distinct components)')
    g = torch.Generator(device='cpu')
    if seed is not None:
      g.manual_seed(int(seed))
    ids = torch.randperm(self.n_components, generator=g)[:n]
    q = self.distribution
    e = torch.randn(n, q.loc.shape[1], generator=g).to(q.loc.device)
    ids = ids.to(q.loc.device)
    return (q.loc[ids] + q.scale[ids] * e).contiguous()


class VampriorVAE(BetaVAE):
  """vamprior.py:136-170 (Tomczak & Welling 2018): a BetaVAE whose latent prior is the Vamprior.  The Monte-Carlo KL of
  the step is log q(z|x) - log p_vamp(z): the fused kernels keep computing the standard-normal KL and the mixture
  kernel adds the correction c = log N(z; 0, I) - log p_vamp(z) (vamprior.hip), so
  kl['kl_<latents>'] = beta * (kl_std + c).  `pseudoinputs`: an explicit [n_components, prod(input_shape)] array for
  W_u (the reference's Vamprior takes it; its VampriorVAE does not pass it on).  Not offered with this prior:
  analytic / forward KL, free_bits, sample_shape other than (), data parallelism."""

  _tril_refusal = "the mixture's components read a diagonal scale"
  _concrete_refusal = "the mixture's components are Gaussian"
  _relaxedbern_refusal = _concrete_refusal

  def __init__(self, n_components: int = 500, pseudoinputs_mean: float = -0.05, pseudoinputs_std: float = 0.01,
               beta: Union[float, Interpolation] = linear(vmin=1e-6, vmax=1., steps=2000, delay_in=0),
               pseudoinputs=None, name='VampriorVAE', **kwargs):
    self.n_components = int(n_components)
    self.pseudoinputs_mean, self.pseudoinputs_std = float(pseudoinputs_mean), float(pseudoinputs_std)
    self._pseudoinputs = pseudoinputs
    ss = kwargs.get('sample_shape', ())
    if isinstance(ss, int) or tuple(ss) != ():
      raise NotImplementedError(f'VampriorVAE with sample_shape={ss!r}: one sample of z per input only')
    self.vamprior: Optional[Vamprior] = None
    super().__init__(beta=beta, name=name, **kwargs)

  def build(self, input_shape):
    ret = super().build(input_shape)
    self.vamprior = Vamprior(self)
    self.latents.prior = self.vamprior
    return ret

  def _reg_options(self) -> dict:
    # (an explicit array initialises W_u once: later engines share the parameter buffer)
    return dict(vamprior_components=self.n_components, pseudoinputs_mean=self.pseudoinputs_mean,
                pseudoinputs_std=self.pseudoinputs_std,
                pseudoinputs=self._pseudoinputs if self._params is None else None)

  def set_elbo_configs(self, analytic=None, reverse=None, free_bits=None, sample_shape=None):
    if analytic or reverse is False or free_bits is not None or sample_shape not in (None, ()):
      raise NotImplementedError('VampriorVAE: analytic / forward KL, free_bits and sample_shape are not offered')
    return super().set_elbo_configs(analytic, reverse, free_bits, sample_shape)

  def elbo_components(self, inputs, training=None, mask=None, eps=None, **kwargs):
    llk, kl = super().elbo_components(inputs, training=training, mask=mask, eps=eps, **kwargs)
    eng = self._engine(_as_tensor(inputs, self.device).shape[0])
    key = f'kl_{self.latents.name}'
    kl[key] = kl[key] + self.beta * eng.vamp_c.clone()
    return llk, kl

  def _step_metrics(self, out, metrics):
    metrics[f'kl_{self.latents.name}'] = out[2] + out[3]   # beta * mean(kl_std + c)

  def sample_prior(self, n: int = 1, seed: int = 1) -> torch.Tensor:
    return self.vamprior.sample(n, seed=seed)

  def _prior_log_prob(self, eng, z, lp):
    eng.pseudo_forward()   # (one encoder pass at batch K, then all n * B samples in chunks)
    eng.vamprior_log_prob(z.reshape(-1, z.shape[-1]), lp.reshape(-1))


# layer name of the quantiser (vq_vae.py:272-281): its variables are VQLatents/codebook and, under the moving average,
# VQLatents/ema_counts and VQLatents/ema_means
VQ_LAYER = 'VQLatents'


class MultinomialPrior:
  """Multinomial(1, logits=0) over the K codes (vector_quantizer.py:110-120): the prior of every code position.  The
  reference's `trainable_prior` creates the logits as a variable, but the KL is taken under stop_gradient: nothing
  ever trains them.  Kept as zeros."""

  def __init__(self, n_codes: int):
    self.n_codes = int(n_codes)
    self.logits = torch.zeros(self.n_codes)

  def log_prob(self, one_hot: torch.Tensor) -> torch.Tensor:
    return -math.log(self.n_codes) * one_hot.sum(-1)


class VectorQuantizedPosterior:
  """vector_quantizer.py (VectorQuantized): codes [B, L, Cs], their assignments [B, L] and nearest codebook rows.
  tensor() / sample() give the value of the straight-through sample, z_q viewed [B, L * Cs]."""

  def __init__(self, codes: torch.Tensor, assignments: torch.Tensor, nearest: torch.Tensor, n_codes: int,
               commitment_weight: float):
    self.codes, self.assignments, self.nearest_codes = codes, assignments, nearest
    self.n_codes, self.commitment_weight = int(n_codes), float(commitment_weight)

  def one_hot(self) -> torch.Tensor:
    return torch.nn.functional.one_hot(self.assignments.long(), self.n_codes).to(torch.float32)

  @property
  def latents_loss(self) -> torch.Tensor:
    return ((self.codes - self.nearest_codes) ** 2).mean()

  @property
  def commitment_loss(self) -> torch.Tensor:
    return self.commitment_weight * self.latents_loss

  def tensor(self) -> torch.Tensor:
    return self.nearest_codes.reshape(self.nearest_codes.shape[0], -1)

  def sample(self, n=None, seed=None) -> torch.Tensor:
    return self.tensor()

  def mean(self) -> torch.Tensor:
    return self.tensor()

  def __array__(self):
    return self.tensor().cpu().numpy()


class VectorQuantizer:
  """vector_quantizer.py:60-200: the configuration of the quantiser and its codebook (held by the model's engines).
  `distance_metric`: 'euclidean' only; `trainable_prior`: accepted, without effect (see MultinomialPrior)."""

  def __init__(self, vae: 'VQVAE', n_codes: int = 64, commitment_weight: float = 0.25,
               distance_metric: str = 'euclidean', trainable_prior: bool = False, ema_decay: float = 0.99,
               ema_update: bool = False, epsilon: float = 1e-5, code_size: Optional[int] = None,
               name: str = 'VectorQuantizer'):
    if str(distance_metric) != 'euclidean':
      raise NotImplementedError(f"distance_metric={distance_metric!r}: the HIP quantiser offers 'euclidean'")
    self._vae = vae
    self.n_codes, self.commitment_weight = int(n_codes), float(commitment_weight)
    self.distance_metric, self.trainable_prior = str(distance_metric), bool(trainable_prior)
    self.ema_decay, self.ema_update, self.epsilon = float(ema_decay), bool(ema_update), float(epsilon)
    self._code_size = None if code_size is None else int(code_size)
    self.name = name
    self.prior = MultinomialPrior(self.n_codes)

  @property
  def code_size(self) -> int:
    return self._vae._engine(1).vq_Cs

  @property
  def codebook(self) -> torch.Tensor:
    """the live [n_codes, code_size] tensor (every engine of the model reads this storage)"""
    return self._vae._engine(1).vq_codebook

  def _assign(self, codes: torch.Tensor):
    eng = self._vae._engine(1)
    c = _as_tensor(codes, self._vae.device).reshape(-1, eng.vq_Cs).contiguous()
    N = c.shape[0]
    idx = torch.empty(N, dtype=torch.int32, device=c.device)
    zq = torch.empty_like(c)
    step = min(N, 65536)
    ws = torch.zeros(eng.lib.odin_vq_workspace(step), dtype=torch.float32, device=c.device)
    m = torch.zeros(2, dtype=torch.float32, device=c.device)
    for i0 in range(0, N, step):
      n = min(step, N - i0)
      eng.lib.odin_vq_assign(c[i0:].data_ptr(), eng.vq_codebook.data_ptr(), idx[i0:].data_ptr(), zq[i0:].data_ptr(),
                             ws.data_ptr(), m.data_ptr(), None, None, n, eng.vq_K, eng.vq_Cs, eng.stream())
    return idx, zq

  def sample_indices(self, codes) -> torch.Tensor:
    """nearest-code indices of codes [..., code_size] (ties: the smallest index)"""
    shp = tuple(np.shape(codes))[:-1]
    return self._assign(codes)[0].reshape(shp)

  def sample_nearest(self, codes) -> torch.Tensor:
    """the nearest codebook rows, same shape as `codes`"""
    return self._assign(codes)[1].reshape(tuple(np.shape(codes)))

  def sample(self, n: int = 1, seed: Optional[int] = None) -> torch.Tensor:
    """n codebook rows at indices drawn uniformly (the prior is Multinomial(1, logits=0))"""
    g = torch.Generator(device='cpu')
    if seed is not None:
      g.manual_seed(int(seed))
    ids = torch.randint(0, self.n_codes, (int(n),), generator=g)
    return self.codebook[ids.to(self._vae.device)].clone()


class VQVAE(BetaVAE):
  """vq_vae.py:249-330 (van den Oord et al. 2017): the encoder's flat output h [B, H] is viewed as L = H / code_size
  codes, each replaced by its nearest codebook row; the decoder reads z_q [B, H] (there is no latent projection).
  loss = -mean llk + beta * L * log K + commitment (+ latents without the moving average).  The reference overrides
  `_elbo`, which its base class never calls, so as shipped the two VQ terms are never added; here elbo_components
  returns them and the step is the one VQVAEStep describes.  `code_size=None`: one code per input
  (what the reference does with the image networks).  Not offered: analytic=False (ValueError, as the reference),
  free_bits, sample_shape other than (), marginal_log_prob (the posterior has no density), data parallelism."""

  _tril_refusal = 'the quantised latent has no Gaussian posterior'
  _concrete_refusal = 'the quantised latent has no posterior distribution'
  _relaxedbern_refusal = _concrete_refusal

  def __init__(self, n_codes: int = 64, commitment_weight: float = 0.25, distance_metric: str = 'euclidean',
               trainable_prior: bool = False, ema_decay: float = 0.99, ema_update: bool = False,
               beta: Union[float, Interpolation] = 1.0, epsilon: float = 1e-5, code_size: Optional[int] = None,
               name='VQVAE', **kwargs):
    analytic = kwargs.pop('analytic', True)
    if not analytic:
      raise ValueError('VQVAE only support analytic KL-divergence.')
    ss = kwargs.get('sample_shape', ())
    if isinstance(ss, int) or tuple(ss) != ():
      raise NotImplementedError(f'VQVAE with sample_shape={ss!r}: one assignment per code only')
    if kwargs.get('free_bits') is not None:
      raise NotImplementedError('VQVAE with free_bits: the KL is the constant L * log K')
    self._quantizer = VectorQuantizer(self, n_codes=n_codes, commitment_weight=commitment_weight,
                                      distance_metric=distance_metric, trainable_prior=trainable_prior,
                                      ema_decay=ema_decay, ema_update=ema_update, epsilon=epsilon, code_size=code_size,
                                      name=VQ_LAYER)
    super().__init__(beta=beta, name=name, analytic=True, **kwargs)

  # ---- the quantiser ----
  @property
  def quantizer(self) -> VectorQuantizer:
    return self._quantizer

  @property
  def codebook(self) -> torch.Tensor:
    return self._quantizer.codebook

  @property
  def ema_update(self) -> bool:
    return self._quantizer.ema_update

  @property
  def ema_counts(self) -> Optional[torch.Tensor]:
    return self._engine(1).vq_ema_counts

  @property
  def ema_means(self) -> Optional[torch.Tensor]:
    return self._engine(1).vq_ema_means

  def _reg_options(self) -> dict:
    q = self._quantizer
    # (the moving-average state lives outside the parameter buffer: later engines share the first one's tensors)
    first = next(iter(self._engines.values()), None)
    return dict(vq_codes=q.n_codes, vq_code_size=q._code_size, vq_commitment=q.commitment_weight, vq_ema=q.ema_update,
                vq_ema_decay=q.ema_decay, vq_epsilon=q.epsilon,
                vq_state=first.vq_state() if (first is not None and q.ema_update) else None)

  def set_elbo_configs(self, analytic=None, reverse=None, free_bits=None, sample_shape=None):
    if analytic is False:
      raise ValueError('VQVAE only support analytic KL-divergence.')
    if free_bits is not None or sample_shape not in (None, ()):
      raise NotImplementedError('VQVAE: free_bits and sample_shape are not offered')
    return super().set_elbo_configs(analytic, reverse, free_bits, sample_shape)

  # ---- forward API ----
  def _posterior(self, eng: VAEEngine) -> VectorQuantizedPosterior:
    B, L, Cs = eng.B, eng.vq_L, eng.vq_Cs
    return VectorQuantizedPosterior(eng.enc.outs[-1].clone().reshape(B, L, Cs), eng.vq_idx.clone().reshape(B, L),
                                    eng.z.clone().reshape(B, L, Cs), eng.vq_K, eng.vq_cw)

  def decode(self, latents, training=None, mask=None, only_decoding=False, **kwargs):
    z = latents.tensor() if isinstance(latents, VectorQuantizedPosterior) else latents
    z = _as_tensor(z, self.device)
    z = z.reshape(z.shape[0], -1).contiguous()
    eng = self._engine(z.shape[0])
    h = eng.run_decoder(z).clone()
    return h if only_decoding else self._observation_dist(h)

  def _vq_terms(self, eng: VAEEngine, m: torch.Tensor) -> Dict[str, torch.Tensor]:
    lat, q = self.latents.name, self._quantizer
    kl = {f'kl_{lat}': torch.full((), self.beta * eng.vq_L * math.log(q.n_codes), dtype=torch.float32,
                                  device=self.device),
          f'commitment_{lat}': q.commitment_weight * m}
    if not q.ema_update:
      kl[f'latents_{lat}'] = m.clone()
    return kl

  def elbo_components(self, inputs, training=None, mask=None, eps=None, **kwargs):
    """llk [B] and the scalar terms kl_<latents> = beta * L * log K, commitment_<latents> and (codebook trained by
    gradient) latents_<latents>; mean(elbo(llk, kl)) = -loss"""
    x = _as_tensor(inputs, self.device)
    eng = self._engine(x.shape[0])
    eng.set_hyper(beta=self.beta, t=self._step)
    eng.forward(x)
    qz_x = self._posterior(eng)
    px_z = self._observation_dist(eng.dec.outs[-1].clone())
    self._last_outputs = (px_z, qz_x)
    llk = {f'llk_{self.observation.name}': eng.llk.clone()}
    return llk, self._vq_terms(eng, eng.out8[4].clone())

  def _step_metrics(self, out, metrics):
    q = self._quantizer
    coef = q.commitment_weight + (0.0 if q.ema_update else 1.0)   # out[3] = coef * m
    m = out[3] / coef if coef > 0 else torch.zeros_like(out[3])
    lat = self.latents.name
    metrics[f'commitment_{lat}'] = q.commitment_weight * m
    if not q.ema_update:
      metrics[f'latents_{lat}'] = m

  def sample_prior(self, n: int = 1, seed: int = 1) -> torch.Tensor:
    """[n, H]: L codebook rows per sample at uniformly drawn indices"""
    eng = self._engine(1)
    return self._quantizer.sample(int(n) * eng.vq_L, seed=seed).reshape(int(n), eng.hdim)

  def marginal_log_prob(self, *args, **kwargs):
    raise NotImplementedError('VQVAE.marginal_log_prob: the quantised posterior has no density')

  # ---- checkpoints: the moving-average form keeps its three tensors outside the parameter buffer ----
  def _extra_checkpoint_variables(self) -> Dict[str, np.ndarray]:
    if not self.ema_update:
      return {}
    eng = self._engine(1)
    return {f'{VQ_LAYER}/{n}': t.detach().cpu().numpy()
            for n, t in zip(('codebook', 'ema_counts', 'ema_means'), eng.vq_state())}

  def _load_extra_checkpoint_variables(self, d: Dict[str, np.ndarray]):
    if not self.ema_update:
      return
    eng = self._engine(1)
    for n, t in zip(('codebook', 'ema_counts', 'ema_means'), eng.vq_state()):
      a = self._find_variable(d, f'{VQ_LAYER}/{n}')
      if tuple(a.shape) != tuple(t.shape):
        raise ValueError(f'{VQ_LAYER}/{n}: checkpoint shape {a.shape} != {tuple(t.shape)}')
      t.copy_(torch.as_tensor(np.asarray(a), dtype=torch.float32, device=self.device))


# ======================================================================================
# FactorVAE
# ======================================================================================
class FactorDiscriminator:
  """factor_discriminator.py:16-235: Flatten -> [Dense(units, relu)]*n -> Dense(1) logit.
  ONE set of flat parameter / gradient / Adam buffers (and one Adam iteration counter) for the
  model; `bind(B1)` adds the launch programs of a batch size: one over B1 samples (TC term
  inside the VAE step: data-gradient only) and one over 2*B1 samples ([z ; permute_dims(z')],
  discriminator step)."""

  def __init__(self, lib, zdim: int, units: Sequence[int], activation: str, device, seed: int):
    self.lib, self.device, self.D = lib, device, zdim
    layers = [('dense', int(u), activation) for u in units] + [('dense', 1, 'linear')]
    self.layout = ParamLayout()
    self.recs, out = build_layers('disc', layers, (zdim,), self.layout)
    self.layout.pad_to(4)
    f32 = dict(dtype=torch.float32, device=device)
    n = self.layout.size
    self.params, self.grads = torch.zeros(n, **f32), torch.zeros(n, **f32)
    self.m, self.v = torch.zeros(n, **f32), torch.zeros(n, **f32)
    g = torch.Generator(device='cpu').manual_seed(seed + 7)
    for key, shp, off in self.layout.entries:
      if key[-1] == 'w':  # glorot_uniform (dense_network default, base_networks.py:968)
        lim = math.sqrt(6.0 / (shp[0] + shp[1]))
        self.params[off:off + int(np.prod(shp))] = \
            ((torch.rand(int(np.prod(shp)), generator=g) * 2 - 1) * lim).to(device)
    self.flag = torch.zeros(1, dtype=torch.int32, device=device)
    self.t = 0  # iterations of the discriminator's own Adam
    self.bound: Dict[int, 'DiscPrograms'] = {}

  @property
  def n_parameters(self):
    return sum(int(np.prod(s)) for _, s, _ in self.layout.entries)

  def bind(self, B1: int, force_dp: bool = False) -> 'DiscPrograms':
    if B1 not in self.bound:
      self.bound[B1] = DiscPrograms(self, B1, force_dp)
    return self.bound[B1]


class DiscPrograms:
  """Launch programs + activation buffers of the discriminator for one half-batch size."""

  def __init__(self, disc: FactorDiscriminator, B1: int, force_dp: bool = False):
    lib, device, zdim = disc.lib, disc.device, disc.D
    f32 = dict(dtype=torch.float32, device=device)
    self.disc, self.B1 = disc, B1
    self.params, self.grads, self.layout = disc.params, disc.grads, disc.layout
    mr = lib.odin_max_slab_rows()
    # (the range words of both programs' gradient tensors in one buffer: cleared once per iteration, reset_ranges)
    nw = len(disc.recs) * RANGE_WORDS
    # (gradient words of the two programs | their activation words, round 5: the layers' inputs keep their 22 bits
    # at any magnitude)
    self.range_words = torch.zeros(4 * nw, dtype=torch.int32, device=device)
    self.prog1 = NetProgram(lib, disc.recs, B1, device, disc.params, disc.grads, mr,
                            range_words=self.range_words[:nw], act_words=self.range_words[2 * nw:3 * nw])
    self.prog2 = NetProgram(lib, disc.recs, 2 * B1, device, disc.params, disc.grads, mr,
                            range_words=self.range_words[nw:2 * nw], act_words=self.range_words[3 * nw:],
                            direct_wgrad=True)
    self.tc = torch.zeros(1, **f32)
    self.dlogit1 = torch.zeros(B1, 1, **f32)
    self.dlogit1_value = None
    self.dz = torch.zeros(B1, zdim, **f32)
    self.zcat = torch.zeros(2 * B1, zdim, **f32)  # [z (step 1's sample) ; permute_dims(z')]
    self.zperm = self.zcat[B1:]
    self.perm = torch.zeros(B1, zdim, dtype=torch.int32, device=device)
    self.world, self.rank = 1, 0
    self.gather = False  # z' is all-gathered before permute_dims (data parallel; also at world size 1 under force_dp)
    import torch.distributed as dist
    if dist.is_available() and dist.is_initialized() and (dist.get_world_size() > 1 or force_dp):
      self.gather = True
      # permute_dims shuffles across the GLOBAL batch (vi/utils.py:262-267): all ranks draw the
      # same [B1_global, D] permutation, z' is all-gathered and every rank gathers its own rows
      self.world, self.rank = dist.get_world_size(), dist.get_rank()
      self.perm = torch.zeros(B1 * self.world, zdim, dtype=torch.int32, device=device)
      self.z2_all = torch.zeros(B1 * self.world, zdim, **f32)
    self.dlogit2 = torch.zeros(2 * B1, 1, **f32)
    self.dtc = torch.zeros(1, **f32)
    self._keep = None
    # the head Dense(K -> 1) with the mean it feeds and its backward as ONE launch per pass (include/odin_hip.h:
    # odin_disc_head_fwd_bwd) instead of forward | mean or dtc_loss | weight gradient | data gradient
    self.fused_head = False
    if len(disc.recs) >= 2 and disc.recs[-1].N == 1 and disc.recs[-1].act == 'linear':
      K = disc.recs[-1].K
      rows = int(lib.odin_disc_head_rows(2 * B1, K))
      if rows > 0 and int(lib.odin_disc_head_rows(B1, K)) > 0:
        self.fused_head = True   # (FactorVAE.fuse_discriminator = False before the first step: the separate launches)
        self.head_slab = torch.empty(rows, K + 1, **f32)
        self.head_ws = torch.zeros(8, dtype=torch.int32, device=device)   # 16 bytes per pass, zero between launches

  m = property(lambda self: self.disc.m)
  v = property(lambda self: self.disc.v)

  def reset_job(self) -> ReduceJob:
    """zero the range words (their producers fold in with atomicMax): a reduction over zero slab rows, riding on
    the iteration's last slab reduction (engine.py: VAEEngine.backward does the same for its own words)"""
    rw = self.range_words
    return ReduceJob(rw.data_ptr(), rw.data_ptr(), rw.numel(), 0, rw.numel(), 0)


H_DALPHA = 10  # discriminator Adam block {alpha_t, beta1, beta2, eps, grad_scale} in the hyper buffer


class FactorVAE(AnnealingVAE):
  """factor_vae.py:99-293.  Each iteration splits the batch in halves (x1, x2):
    step 1 (VAE params, fit's Adam): loss = -mean(llk - beta_t*kl) + tc_coef*mean(D(z)),
            the gradient flows through D into z (total_correlation, factor_discriminator.py:169-198);
    step 2 (discriminator params, Adam(1e-5, .5, .9)): dtc_loss of D(z) and
            D(permute_dims(z')) with z' = encode(x2) (factor_discriminator.py:200-235).
  On one GPU the whole iteration (both steps, both optimisers) is replayed as ONE HIP graph
  when `use_graph` / `fit(compile_graph=True)`."""

  _tril_refusal = 'its forward-only second engine shares range words, which the triangular path does not offer'
  _concrete_refusal = 'its forward-only second engine shares range words, which the relaxed one-hot path does not offer'
  _relaxedbern_refusal = 'its forward-only second engine shares range words, which the relaxed Bernoulli path does not offer'

  def __init__(self, discriminator_units: Sequence[int] = (1000,) * 5, discriminator_optim=None,
               activation: str = 'relu', batchnorm: bool = False, tc_coef: float = 7.0,
               maximize_tc: bool = False, name='FactorVAE', **kwargs):
    if batchnorm:
      raise NotImplementedError('batchnorm=True is outside the HIP path (reference default False)')
    super().__init__(name=name, **kwargs)
    self.tc_coef = float(tc_coef) * (-1.0 if maximize_tc else 1.0)
    self.disc_units, self.disc_act = tuple(discriminator_units), activation
    self.disc_lr, self.disc_b1, self.disc_b2 = 1e-5, 0.5, 0.9
    if discriminator_optim is not None:  # dict(learning_rate=, beta_1=, beta_2=) accepted
      self.disc_lr = float(discriminator_optim.get('learning_rate', self.disc_lr))
      self.disc_b1 = float(discriminator_optim.get('beta_1', self.disc_b1))
      self.disc_b2 = float(discriminator_optim.get('beta_2', self.disc_b2))
    self._is_pretraining = False
    self._disc_state: Optional[FactorDiscriminator] = None
    self._fgraphs: Dict[tuple, Any] = {}

  @property
  def is_pretraining(self):
    return self._is_pretraining

  def pretrain(self):
    self._is_pretraining = True
    return self

  def finetune(self):
    self._is_pretraining = False
    return self

  @property
  def discriminator(self) -> FactorDiscriminator:
    if self._disc_state is None:
      eng = self._engine(1)
      self._disc_state = FactorDiscriminator(eng.lib, self.zdim, self.disc_units, self.disc_act,
                                             self.device, self.seed)
      from .dist import broadcast_parameters
      broadcast_parameters(self._disc_state.params, src=0)
    return self._disc_state

  def _disc_names(self):
    """[(checkpoint name, flat offset, shape)] of the discriminator's variables: Keras names of
    `dense_network` inside the `FactorDiscriminator` sub-layer (factor_discriminator.py:60-95)."""
    D = self.discriminator
    return [(f"discriminator/dense_{key[1]}/{'kernel' if key[-1] == 'w' else 'bias'}", off, shp)
            for key, shp, off in D.layout.entries]

  def _extra_checkpoint_variables(self) -> Dict[str, np.ndarray]:
    """The reference keeps `self.discriminator` (a Keras layer) and `self.disc_optimizer` as
    attributes of the model (factor_vae.py:137-160), so `save_weights` tracks both: the
    discriminator's kernels / biases, its Adam's iteration count and moment slots.  A restored
    FactorVAE continues with the SAME discriminator and bias correction."""
    D = self.discriminator
    W = {}
    for name, off, shp in self._disc_names():
      n = int(np.prod(shp))
      W[name] = D.params[off:off + n].view(shp).detach().cpu().numpy()
      W[f'disc_optimizer/{name}/m'] = D.m[off:off + n].view(shp).detach().cpu().numpy()
      W[f'disc_optimizer/{name}/v'] = D.v[off:off + n].view(shp).detach().cpu().numpy()
    W['disc_optimizer/iter'] = np.asarray(D.t, np.int64)
    return W

  def _load_extra_checkpoint_variables(self, d: Dict[str, np.ndarray]):
    names = self._disc_names()
    have = [any(n == nm or n.endswith('/' + nm) for n in d) for nm, _, _ in names]
    if not any(have):
      if self._is_pretraining:
        return  # a checkpoint of the pretraining phase may predate the discriminator
      raise KeyError('the checkpoint holds no discriminator variables (discriminator/dense_*/kernel): '
                     'a FactorVAE restored from it would continue with a re-initialised discriminator; '
                     'call pretrain() first if that is intended')
    D = self.discriminator
    as_t = lambda a: torch.as_tensor(np.asarray(a), dtype=torch.float32, device=self.device)
    for name, off, shp in names:
      n = int(np.prod(shp))
      a = self._find_variable(d, name)
      if tuple(a.shape) != tuple(shp):
        raise ValueError(f'{name}: checkpoint shape {a.shape} != {tuple(shp)}')
      D.params[off:off + n].view(shp).copy_(as_t(a))
      for slot, buf in (('m', D.m), ('v', D.v)):
        buf[off:off + n].view(shp).copy_(as_t(self._find_variable(d, f'disc_optimizer/{name}/{slot}')))
    D.t = int(self._find_variable(d, 'disc_optimizer/iter'))

  def _discriminator(self, B1: int) -> DiscPrograms:
    dp = self.discriminator.bind(B1, bool(getattr(self, 'force_dp', False)))
    eng = self._engine(B1)
    if eng.z.data_ptr() != dp.zcat.data_ptr():
      # step 1's cached sample IS the first half of the discriminator step's input: the engine
      # writes z there directly (no per-iteration copy); must happen before any graph capture
      assert not getattr(eng, '_graphs', None), 'bind the discriminator before capturing graphs'
      eng.z = dp.zcat[:B1]
    return dp

  # -- the two steps, returning device scalars ------------------------------------------
  def _set_hyper(self, eng, disc, lr, use_tc, training, when_skip_update: int = 0):
    h_extra = None
    if training and not self._is_pretraining:
      t = disc.disc.t + 1
      a = self.disc_lr * math.sqrt(1 - self.disc_b2 ** t) / (1 - self.disc_b1 ** t)
      # (grad_scale 1 / world: the discriminator's bucket is SUMMED over the ranks, its loss is a mean
      # over the global batch)
      h_extra = (a, self.disc_b1, self.disc_b2, 1e-7, 1.0 / eng.world_size)
    eng.set_hyper(lr=lr, beta=self.beta, tc_coef=self.tc_coef if use_tc else 0.0, extra=h_extra,
                  skip_enable=self._step >= int(when_skip_update or 0))

  def _program(self, eng, eng2, disc, x1, x2, eps, eps2, perm, training, use_tc, pol,
               aggregate_gradients):
    """The launch program of one FactorVAE iteration: [('k', fn) kernels | ('c', fn) collective]
    (engine.VAEEngine.step_program).  On one GPU there is no 'c' entry: one graph per iteration.  Data
    parallel: A | all-reduce (VAE bucket) | B | all-gather (z' for the global permute_dims) | C |
    all-reduce (discriminator bucket) | D."""
    lib, B1 = eng.lib, disc.B1
    dp = eng.is_dp
    P = []
    # A/B switch (bench.py --no-fused-disc): the head's launches and permute_dims as round 5 issued them
    fuse = bool(getattr(self, 'fuse_discriminator', True))
    fused_head = disc.fused_head and fuse
    # the discriminator's update with its last small gradient pieces formed inside the Adam launch (odin_adam_step_fold:
    # the first layer's thin-K weight gradient, the sum of the head's slab rows, the range-word reset) -- one GPU only: a
    # data-parallel step all-reduces the finished gradient buffer first
    r0, rh = disc.prog2.recs[0], disc.prog2.recs[-1]
    fold_adam = bool(fused_head and training and not dp and r0.kind == 'dense' and r0.K <= 32 and
                     ((r0.K + 1) * r0.N) % 4 == 0 and r0.w_off % 4 == 0 and r0.b_off == r0.w_off + r0.K * r0.N and
                     rh.w_off % 4 == 0 and rh.b_off == rh.w_off + rh.K)

    # The discriminator's pass over z (TC estimate + its gradient wrt z: twelve small launches, ~96 us at batch 128, none
    # of which fills the chip) depends on z alone and is needed again only by the ENCODER's backward pass: `overlap_disc`
    # runs it on a side stream beside the decoder's forward pass and fused tail.  Measured (round 6, same-call A/B,
    # `bench.py --overlap-disc`): 0.755 ms per iteration against 0.735 on one stream -- the decoder's launches hold
    # every CU with 8 waves and ~100 KB of LDS, the forked branch of the captured graph waits for them and then delays the
    # join -- so it is OFF by default, like the engine's other overlap options.
    side = getattr(eng, 'side_stream', None)
    overlap = bool(getattr(self, 'overlap_disc', False)) and use_tc and training and side is not None

    def disc_pass(st):
      P1 = disc.prog1
      if fused_head:
        n = len(P1.recs)
        h = P1.forward(eng.z, st, upto=n - 1)
        lib.odin_disc_head_fwd_bwd(h.data_ptr(), P1.w(n - 1).data_ptr(), P1.b(n - 1).data_ptr(), P1.outs[n - 1].data_ptr(),
                                   0, disc.dlogit1.data_ptr(), None, disc.tc.data_ptr(), ACT[P1.recs[n - 2].act],
                                   P1.gouts[n - 2].data_ptr(), P1.word(n - 2), None, None, disc.head_ws.data_ptr(), B1,
                                   P1.recs[n - 1].K, st)
        P1.backward(eng.z, P1.gouts[n - 2], st, dx_out=disc.dz, data_only=True, last=n - 2)
        return
      lg = P1.forward(eng.z, st)
      lib.odin_mean(lg.data_ptr(), B1, disc.tc.data_ptr(), st)
      P1.backward(eng.z, disc.dlogit1, st, dx_out=disc.dz, data_only=True)

    def step1():  # ELBO with the discriminator's TC estimate, backward
      st = eng.stream()
      if overlap:
        cur = torch.cuda.current_stream(self.device)

        def fork_disc():
          ev = torch.cuda.Event()
          ev.record(cur)
          side.wait_event(ev)
          disc_pass(side.cuda_stream)

        eng.forward(x1, eps, finalize=False, after_latent=fork_disc)
        cur.wait_stream(side)   # (dz and the TC mean are complete before the backward pass / the finalisation)
      else:
        eng.forward(x1, eps, finalize=False)
      extra = None
      # the ELBO finalisation (llk[B], loss, mean terms: nothing in the backward pass reads them) rides in the first
      # launch of the VAE optimiser's update when one follows (engine.adam: _fin_pending), as in the plain VAE step
      ride = training
      if use_tc:
        if not overlap:
          disc_pass(st)
        if ride:
          eng._fin_pending = (eng._llk_part_used.data_ptr(), eng.n_part, disc.tc.data_ptr())
        else:
          eng.finalize(tc_ptr=disc.tc.data_ptr())
        extra = disc.dz
        if not training or self._is_pretraining:  # (no discriminator step behind this one to clear the words)
          lib.odin_range_reset(disc.range_words.data_ptr(), disc.range_words.numel() // RANGE_WORDS, st)
      elif ride:
        eng._fin_pending = (eng._llk_part_used.data_ptr(), eng.n_part, None)
      else:
        eng.finalize()
      if training:
        # the gradient norm's stage-1 sums ride in the slab reduction when the update follows at once with no per-tensor
        # policy in between (engine.VAEEngine.step_program does the same for the plain step)
        eng._fuse_norm_now = bool(fuse and not dp and not aggregate_gradients and pol[1] is None and pol[2] is None and
                                  pol[3] is None and (pol[0] is not None or pol[4]) and eng.fuse_norm)
        try:
          eng.backward(extra_dz=extra)
        finally:
          eng._fuse_norm_now = False

    P.append(('k', step1))
    if training and dp:
      P.append(('c', eng.allreduce))
    if training and not aggregate_gradients:
      P.append(('k', lambda: eng._update(pol)))
    # ---- step 2: discriminator (skipped while pretraining, factor_vae.py:279) ----
    if not self._is_pretraining:
      def encode2():
        st = eng.stream()
        eng2.run_encoder(x2, eps2)  # z' with the encoder as step 1 left it
        if perm is None and not disc.gather and fuse:   # (the permutation and permute_dims(z') in one launch)
          lib.odin_random_permute_dims(disc.perm.data_ptr(), eng2.z.data_ptr(), disc.zperm.data_ptr(), B1, self.zdim,
                                       self.seed + 11, eng.hp(N_HYPER), st)
        elif perm is None:
          lib.odin_random_perm(disc.perm.data_ptr(), B1 * disc.world, self.zdim, self.seed + 11,
                               eng.hp(N_HYPER), st)

      P.append(('k', encode2))
      if disc.gather:
        P.append(('c', lambda: eng._comm().all_gather(disc.z2_all.view(-1), eng2.z.view(-1))))

      def disc_step():
        st = eng.stream()
        if disc.gather:
          src, prm = disc.z2_all, disc.perm[disc.rank * B1:(disc.rank + 1) * B1]
        else:
          src, prm = eng2.z, disc.perm
        if perm is not None or disc.gather or not fuse:
          lib.odin_permute_dims(src.data_ptr(), prm.data_ptr(), disc.zperm.data_ptr(), B1,
                                self.zdim, st)
        P2 = disc.prog2
        if fused_head:
          n = len(P2.recs)
          r = P2.recs[n - 1]
          h = P2.forward(disc.zcat, st, upto=n - 1)
          hrows = C.c_int(0)
          lib.odin_disc_head_fwd_bwd(h.data_ptr(), P2.w(n - 1).data_ptr(), P2.b(n - 1).data_ptr(), P2.outs[n - 1].data_ptr(),
                                     1, None, disc.dlogit2.data_ptr(), disc.dtc.data_ptr(), ACT[P2.recs[n - 2].act],
                                     P2.gouts[n - 2].data_ptr() if training else None, P2.word(n - 2),
                                     disc.head_slab.data_ptr(), C.byref(hrows), disc.head_ws[4:].data_ptr(), 2 * B1, r.K, st)
          if training and fold_adam:
            jobs = P2.backward(disc.zcat, P2.gouts[n - 2], st, last=n - 2, first=1)
            if jobs:   # (none with the 1000-unit stack: its hidden layers write their gradients themselves)
              arr = (ReduceJob * len(jobs))(*jobs)
              disc._keep = arr
              lib.odin_slab_reduce(arr, len(jobs), st)
            return
          if training:
            jobs = P2.backward(disc.zcat, P2.gouts[n - 2], st, last=n - 2)
            jobs.append(ReduceJob(disc.head_slab.data_ptr(), disc.grads[r.w_off:].data_ptr(), r.K + 1, hrows.value, r.K + 1, 0))
        else:
          lg2 = P2.forward(disc.zcat, st)
          lib.odin_dtc_loss_fwd_bwd(lg2.data_ptr(), lg2[B1:].data_ptr(), disc.dtc.data_ptr(),
                                    disc.dlogit2.data_ptr(), disc.dlogit2[B1:].data_ptr(), B1, st)
          if training:
            jobs = P2.backward(disc.zcat, disc.dlogit2, st)
        if training:
          jobs.append(disc.reset_job())
          arr = (ReduceJob * len(jobs))(*jobs)
          disc._keep = arr
          lib.odin_slab_reduce(arr, len(jobs), st)

      P.append(('k', disc_step))
      if training:
        if dp:
          P.append(('c', lambda: eng._comm().all_reduce(disc.grads)))
        def disc_update():
          if fold_adam:
            P2 = disc.prog2
            fo = _lib.AdamFold(disc.zcat.data_ptr(), P2.gouts[0].data_ptr(), 2 * B1, r0.K, r0.N, r0.w_off,
                               disc.head_slab.data_ptr(), disc.head_slab.shape[0], rh.K + 1, rh.K + 1, rh.w_off,
                               disc.range_words.data_ptr(), disc.range_words.numel())
            disc._fold_keep = fo
            lib.odin_adam_step_fold(disc.params.data_ptr(), disc.grads.data_ptr(), disc.m.data_ptr(), disc.v.data_ptr(),
                                    disc.params.numel(), eng.hp(H_DALPHA), C.byref(fo), eng.stream())
            return
          lib.odin_adam_step_flat(disc.params.data_ptr(), disc.grads.data_ptr(), disc.m.data_ptr(), disc.v.data_ptr(),
                                  disc.params.numel(), eng.hp(H_DALPHA), None, 0.0, None, eng.stream())

        P.append(('k', disc_update))
    if training and aggregate_gradients:
      P.append(('k', lambda: eng._update(pol)))
    return P

  def _iteration(self, *args):
    """eager launch of one iteration on the current stream"""
    for _, fn in self._program(*args):
      fn()

  def optimize(self, inputs, training: bool = True, optimizer=None, learning_rate=1e-4,
               clipnorm=None, clipvalue=None, global_clipnorm=None, skip_update_threshold=None,
               when_skip_update: int = 0, nan_gradients_policy: str = 'skip',
               allow_none_gradients=False, aggregate_gradients=False, track_gradients=False,
               eps=None, eps2=None, perm=None, use_graph: bool = False, snapshot: bool = True, **kwargs):
    """Networks.optimize over FactorVAE.train_steps (factor_vae.py:239-287): the gradient
    policies apply to the VAE step's gradients (the discriminator step has its own optimiser
    and, as in the reference's default call, no clipping is configured for it separately --
    the same clip arguments are NOT applied to it here; state otherwise if you need them)."""
    x = _as_tensor(inputs, self.device)
    assert x.shape[0] % 2 == 0, 'FactorVAE splits the batch in two halves'
    if self.n_samples != 1:
      raise NotImplementedError('FactorVAE on the HIP path draws one posterior sample per input '
                                '(sample_shape=()); the batch-tiling of VariationalAutoencoder.optimize '
                                'is not wired through the two-step iteration')
    B1 = x.shape[0] // 2
    eng, disc = self._engine(B1), self._discriminator(B1)
    eng2 = self._engine_x2(B1)
    disc.dtc = eng.out8[4:5]   # (beside out4: one device-to-device copy snapshots the iteration's scalars)
    if training:
      self._step += 1
    eng.step_count = self._step
    eng2.hyper = eng.hyper  # one hyper buffer (RNG step, beta) for both halves
    use_tc = not (self._is_pretraining and training)
    # (Round 6, tried and dropped: two device rows for the iteration's scalars, one captured graph per row, the row of
    # iteration t + 1 copied on a side stream while iteration t runs and the main stream waiting on its event only --
    # to take the 80-byte copy and the gaps around it, 13 us, off the critical path.  Same-call A/B: 0.684 ms against
    # 0.649 with the plain stream-ordered copy; the cross-stream waits cost more than the copy.)
    self._set_hyper(eng, disc, self._lr(learning_rate), use_tc, training, when_skip_update)
    val = self.tc_coef / (B1 * eng.world_size)
    if disc.dlogit1_value != val:
      disc.dlogit1.fill_(val)
      disc.dlogit1_value = val
    if perm is not None:
      disc.perm.copy_(torch.as_tensor(perm, dtype=torch.int32, device=self.device))
    pol = (global_clipnorm, clipnorm, clipvalue, skip_update_threshold,
           nan_gradients_policy != 'ignore')
    te = None if eps is None else _as_tensor(eps, self.device)
    te2 = None if eps2 is None else _as_tensor(eps2, self.device)
    graphable = use_graph and self.device.type == 'cuda'
    if graphable:
      self._graph_iteration(eng, eng2, disc, x, te, te2, perm is not None, training, use_tc, pol,
                            aggregate_gradients)
    else:
      x1, x2 = x[:B1], x[B1:]
      self._iteration(eng, eng2, disc, x1, x2, te, te2, perm, training, use_tc, pol,
                      aggregate_gradients)
    if training and not self._is_pretraining:
      disc.disc.t += 1
    # (snapshot=False: the returned scalars are views of the buffer the NEXT iteration overwrites -- what
    # VAEEngine.train_step returns; saves the per-iteration device-to-device copy of a tight training loop)
    out = eng.out8.clone() if snapshot else eng.out8
    metrics = {f'elbo/llk_{self.observation.name}': out[1],
               f'elbo/kl_{self.latents.name}': out[2], 'elbo/tc': out[3]}
    if not self._is_pretraining:
      metrics['disc/dtc_loss'] = out[4]
    if training and track_gradients:
      for k, g in eng.grad_views().items():
        metrics['_grad/elbo/' + self.variable_name(k)] = g.clone()
    return out[0], metrics

  def _graph_iteration(self, eng, eng2, disc, x, eps, eps2, explicit_perm, training, use_tc, pol,
                       aggregate_gradients):
    """HIP graphs per (batch size, configuration): both steps, both Adams -- ONE graph on one GPU, the
    kernel segments between the collectives under data parallelism (dist.SegmentedGraph)."""
    from .dist import SegmentedGraph
    B1 = disc.B1
    key = (B1, pol, eps is not None, eps2 is not None, explicit_perm, training, use_tc,
           aggregate_gradients, self._is_pretraining, eng.analytic, eng.free_bits,
           bool(getattr(self, 'fuse_discriminator', True)))
    if key not in self._fgraphs:
      xs = self.input_buffer(x.shape[0])
      if x.data_ptr() != xs.data_ptr():
        xs.copy_(x)
      if eps is not None:
        eng.eps.copy_(eps)
      if eps2 is not None:
        eng2.eps.copy_(eps2)
      sg = SegmentedGraph(self.device, self._program(
          eng, eng2, disc, xs[:B1], xs[B1:], eng.eps if eps is not None else None,
          eng2.eps if eps2 is not None else None, True if explicit_perm else None, training, use_tc,
          pol, aggregate_gradients))
      cap = torch.cuda.Stream(self.device)
      cap.wait_stream(torch.cuda.current_stream(self.device))
      D = disc.disc
      saved = [t.clone() for t in (eng.params, eng.m, eng.v, D.params, D.m, D.v, eng.flag,
                                   eng.skipped_update)]
      with torch.cuda.stream(cap):
        sg.run_eager()  # warm-up outside capture; must not count
        for t, sv in zip((eng.params, eng.m, eng.v, D.params, D.m, D.v, eng.flag,
                          eng.skipped_update), saved):
          t.copy_(sv)
      torch.cuda.current_stream(self.device).wait_stream(cap)
      sg.capture(cap)
      self._fgraphs[key] = (sg, xs)
    sg, xs = self._fgraphs[key]
    if x.data_ptr() != xs.data_ptr():
      xs.copy_(x, non_blocking=True)
    if eps is not None:
      eng.eps.copy_(eps, non_blocking=True)
    if eps2 is not None:
      eng2.eps.copy_(eps2, non_blocking=True)
    sg.replay()

  def input_buffer(self, batch_size: int) -> torch.Tensor:
    """Static [B, H, W, C] tensor every captured iteration graph of this batch size reads: a data pipeline that
    writes the next batch straight into it (and passes it to optimize) saves the per-iteration device-to-device copy."""
    if not hasattr(self, '_xs'):
      self._xs = {}
    B = int(batch_size)
    if B not in self._xs:
      self._xs[B] = torch.empty((B,) + tuple(self.input_shape), dtype=torch.float32, device=self.device)
    return self._xs[B]

  def _engine_x2(self, B1: int) -> VAEEngine:
    key = -B1
    if key not in self._engines:
      self._engine(B1)
      self._engines[key] = VAEEngine(self.encoder.layers, self.decoder.layers, self.input_shape,
                                     self.zdim, B1, self.device,
                                     observation=self.observation.posterior,
                                     analytic=self.analytic, free_bits=self.free_bits,
                                     lib=self._lib, params=self._params,
                                     seed=self.seed + 1000003 + self._rank(),
                                     range_words=self._engines[B1].range_words)
    return self._engines[key]

  def total_correlation(self, qz_x, training=None):
    z = _as_tensor(qz_x.tensor() if isinstance(qz_x, MVNDiagPosterior) else qz_x, self.device)
    disc = self._discriminator(z.shape[0])
    lg = disc.prog1.forward(z, self._engine(z.shape[0]).stream())
    return self.tc_coef * lg.mean()

  def dtc_loss(self, qz_x, qz_xprime=None, training=None, perm=None):
    z = _as_tensor(qz_x.tensor() if isinstance(qz_x, MVNDiagPosterior) else qz_x, self.device)
    zp = z if qz_xprime is None else _as_tensor(
        qz_xprime.tensor() if isinstance(qz_xprime, MVNDiagPosterior) else qz_xprime, self.device)
    B1 = z.shape[0]
    disc, eng = self._discriminator(B1), self._engine(B1)
    lib, st = eng.lib, eng.stream()
    if perm is None:
      lib.odin_random_perm(disc.perm.data_ptr(), B1, self.zdim, self.seed + 11, None, st)
    else:
      disc.perm.copy_(torch.as_tensor(perm, dtype=torch.int32, device=self.device))
    zp = zp.clone()  # (zp may alias the buffer permute_dims writes)
    disc.zcat[:B1].copy_(z)
    lib.odin_permute_dims(zp.data_ptr(), disc.perm.data_ptr(), disc.zperm.data_ptr(), B1,
                          self.zdim, st)
    lg2 = disc.prog2.forward(disc.zcat, st)
    lib.odin_dtc_loss_fwd_bwd(lg2.data_ptr(), lg2[B1:].data_ptr(), disc.dtc.data_ptr(),
                              disc.dlogit2.data_ptr(), disc.dlogit2[B1:].data_ptr(), B1, st)
    return disc.dtc[0].clone()


# ======================================================================================
# TwoStageVAE
# ======================================================================================
SKIP_HEAD_DMAX = 128    # include/odin_hip.h: odin_skip_head_fwd (Dx and N / 2)
SKIP_HEAD_HMAX = 4096   # (H, a multiple of 4)
# stage-2 hyper block (DEVICE floats): Adam {alpha_t, beta1, beta2, eps, grad_scale} | {beta = 1, tc_coef = 0} of
# odin_elbo_finalize | 1 / B (the heads' `scale`, the latent kernel's `klw`) | the step (int32, odin_rng_normal)
S2_ALPHA, S2_BETA, S2_INVB, S2_STEP, S2_HYPER = 0, 5, 7, 8, 12


class Stage2Network:
  """two_stage_vae.py:68-97: encoder2 = z -> [Dense(units_i, act)] -> Concatenate([z, h]), latents2 = MVNDiagLatents(Du),
  decoder2 = u -> [Dense(units[::-1]_i, act)] -> Concatenate([u, g]), observation2 = MVNDiagLatents(D).  ONE set of flat
  parameter / gradient / Adam buffers with its own iteration count (the second optimiser); `bind(B)` adds the launch
  programs of a batch size.  The two projections over a concatenation are the skip heads of stage2.hip."""

  def __init__(self, lib, zdim: int, zdim2: int, units: Sequence[int], activation: str, device, seed: int):
    units = tuple(int(u) for u in units)
    self.check_limits(zdim, zdim2, units)
    self.lib, self.device, self.D, self.Du, self.units, self.act = lib, device, int(zdim), int(zdim2), units, activation
    self.layout = ParamLayout()
    self.enc_recs, _ = build_layers('encoder2', [('dense', u, activation) for u in units], (self.D,), self.layout)
    self.dec_recs, _ = build_layers('decoder2', [('dense', u, activation) for u in units[::-1]], (self.Du,), self.layout)
    self.He, self.Hd = units[-1], units[0]
    # (kernel | bias contiguous: one slab reduction writes a head's (dW | db) in place; the kernels start on 16-byte
    # boundaries: the heads then read them with 16-byte loads)
    self.lat_shape, self.obs_shape = (self.D + self.He, 2 * self.Du), (self.Du + self.Hd, 2 * self.D)
    self.layout.pad_to(4)
    self.lat_w_off = self.layout.add(('latents2', 'w'), self.lat_shape)
    self.lat_b_off = self.layout.add(('latents2', 'b'), (2 * self.Du,))
    self.layout.pad_to(4)
    self.obs_w_off = self.layout.add(('observation2', 'w'), self.obs_shape)
    self.obs_b_off = self.layout.add(('observation2', 'b'), (2 * self.D,))
    self.layout.pad_to(4)
    f32 = dict(dtype=torch.float32, device=device)
    n = self.layout.size
    self.params, self.grads = torch.zeros(n, **f32), torch.zeros(n, **f32)
    self.m, self.v = torch.zeros(n, **f32), torch.zeros(n, **f32)
    g = torch.Generator(device='cpu').manual_seed(seed + 13)
    for key, shp, off in self.layout.entries:
      if key[-1] != 'w':   # zero biases
        continue
      cnt = int(np.prod(shp))
      if key[0] in ('latents2', 'observation2'):   # DistributionDense: glorot_normal (dense_distribution.py:124)
        w = torch.randn(cnt, generator=g) * math.sqrt(2.0 / (shp[0] + shp[1]))
      else:                                        # Keras Dense default: glorot_uniform
        w = (torch.rand(cnt, generator=g) * 2 - 1) * math.sqrt(6.0 / (shp[0] + shp[1]))
      self.params[off:off + cnt] = w.to(device)
    self.flag = torch.zeros(1, dtype=torch.int32, device=device)
    self.t = 0   # iterations of the second stage's own Adam
    self.bound: Dict[int, 'Stage2Programs'] = {}

  @staticmethod
  def check_limits(zdim: int, zdim2: int, units: Sequence[int]):
    """the regime of odin_skip_head_fwd / _bwd (include/odin_hip.h), named when the model is built"""
    if len(units) < 1:
      raise ValueError('TwoStageVAE: stage2_units must name at least one hidden layer (the skip heads read the last one)')
    for what, d in (('the first stage\'s zdim', zdim), ('stage2_zdim', zdim2)):
      if not 1 <= int(d) <= SKIP_HEAD_DMAX:
        raise ValueError(f'TwoStageVAE: {what} = {d} is outside the skip heads\' limit 1 <= D <= {SKIP_HEAD_DMAX}')
    for what, h in (('stage2_units[-1]', units[-1]), ('stage2_units[0]', units[0])):
      if h < 4 or h % 4 != 0 or h > SKIP_HEAD_HMAX:
        raise ValueError(f'TwoStageVAE: {what} = {h} is outside the skip heads\' limit: the hidden width a head reads '
                         f'must be a multiple of 4 in [4, {SKIP_HEAD_HMAX}]')
    if any(u < 1 for u in units):
      raise ValueError(f'TwoStageVAE: stage2_units = {tuple(units)} must be positive')

  @property
  def n_parameters(self):
    return sum(int(np.prod(s)) for _, s, _ in self.layout.entries)

  def names(self):
    """[(checkpoint name, flat offset, shape)]: the Keras names of the four stage-2 layers (two_stage_vae.py:79-92)"""
    out = []
    for key, shp, off in self.layout.entries:
      suffix = 'kernel' if key[-1] == 'w' else 'bias'
      if key[0] in ('latents2', 'observation2'):
        out.append((f'{key[0]}/{suffix}', off, shp))
      else:
        out.append((f"{key[0]}/{'Encoder2' if key[0] == 'encoder2' else 'Decoder2'}_{key[1]}/{suffix}", off, shp))
    return out

  def bind(self, B: int) -> 'Stage2Programs':
    if B not in self.bound:
      self.bound[B] = Stage2Programs(self, B)
    return self.bound[B]


class Stage2Programs:
  """Launch programs + activation buffers of the second stage for one batch size: two NetPrograms (the dense stacks),
  the two skip heads, odin_latent_fwd / _bwd for q(u|z), odin_slab_reduce and the second optimiser's Adam."""

  def __init__(self, net: Stage2Network, B: int):
    lib, device, D, Du = net.lib, net.device, net.D, net.Du
    f32 = dict(dtype=torch.float32, device=device)
    self.net, self.B = net, B
    mr = lib.odin_max_slab_rows()
    ne, nd = len(net.enc_recs) * RANGE_WORDS, len(net.dec_recs) * RANGE_WORDS
    # (gradient words of the two stacks | their activation words: cleared once per step, reset_job)
    self.range_words = torch.zeros(2 * (ne + nd), dtype=torch.int32, device=device)
    rw = self.range_words
    self.enc = NetProgram(lib, net.enc_recs, B, device, net.params, net.grads, mr, range_words=rw[:ne],
                          act_words=rw[ne + nd:2 * ne + nd])
    self.dec = NetProgram(lib, net.dec_recs, B, device, net.params, net.grads, mr, range_words=rw[ne:ne + nd],
                          act_words=rw[2 * ne + nd:])
    # (the heads' backward leaves dh = the stacks' top gradients with their range words)
    self.enc.set_top_word(True)
    self.dec.set_top_word(True)
    self.p2, self.dp2 = torch.zeros(B, 2 * Du, **f32), torch.zeros(B, 2 * Du, **f32)   # q(u|z): (loc | raw scale)
    self.eps2, self.u = torch.zeros(B, Du, **f32), torch.zeros(B, Du, **f32)
    self.kl2, self.fbmask = torch.zeros(B, **f32), torch.zeros(B, **f32)
    self.du_head, self.du_stack = torch.zeros(B, Du, **f32), torch.zeros(B, Du, **f32)
    self.po, self.dpo = torch.zeros(B, 2 * D, **f32), torch.zeros(B, 2 * D, **f32)     # p(z|u): (loc | raw scale)
    self.llk_raw, self.llk = torch.zeros(B, **f32), torch.zeros(B, **f32)
    self.eps3, self.zs = torch.zeros(B, D, **f32), torch.zeros(B, D, **f32)            # a sample of q(z|u)
    self.kl_unused, self.mask_unused = torch.zeros(B, **f32), torch.zeros(B, **f32)
    self.out4 = torch.zeros(4, **f32)   # loss | mean llk | mean kl | 0
    self.hyper = torch.zeros(S2_HYPER, **f32)
    self._hyper_host = torch.zeros(S2_HYPER, dtype=torch.float32)
    self.ws, self.gnorm2 = torch.zeros(1024, **f32), torch.zeros(1, **f32)
    rows = C.c_int(0)
    lib.odin_skip_head_bwd(None, None, None, None, 0, None, None, None, None, C.byref(rows), B, D, net.He, 2 * Du, None)
    self.lat_slab = torch.empty(rows.value, net.lat_shape[0] * net.lat_shape[1] + 2 * Du, **f32)
    lib.odin_skip_head_bwd(None, None, None, None, 0, None, None, None, None, C.byref(rows), B, Du, net.Hd, 2 * D, None)
    self.obs_slab = torch.empty(rows.value, net.obs_shape[0] * net.obs_shape[1] + 2 * D, **f32)
    self._words_dirty = False
    self._keep = None

  def hp(self, idx: int) -> int:
    return self.hyper.data_ptr() + 4 * idx

  def stream(self):
    if self.net.device.type == 'cuda':
      return torch.cuda.current_stream(self.net.device).cuda_stream
    return None

  def set_hyper(self, step: int, optim: Optional[dict] = None):
    """host scalars -> device; `optim`: the second optimiser's (learning_rate, beta_1, beta_2, epsilon) for the update
    that follows (its bias correction reads the network's own iteration count)"""
    h = self._hyper_host
    h.zero_()
    if optim is not None:
      t = self.net.t + 1
      b1, b2 = optim['beta_1'], optim['beta_2']
      h[S2_ALPHA] = optim['learning_rate'] * math.sqrt(1.0 - b2 ** t) / (1.0 - b1 ** t)
      h[S2_ALPHA + 1], h[S2_ALPHA + 2], h[S2_ALPHA + 3], h[S2_ALPHA + 4] = b1, b2, optim['epsilon'], 1.0
    h[S2_BETA] = 1.0   # (beta is not applied in stage 2: TwoStageVAE.elbo_components bypasses BetaVAE's scaling)
    h[S2_INVB] = 1.0 / self.B
    h[S2_STEP:].view(torch.int32)[0] = int(step)
    self.hyper.copy_(h)

  def _w(self, off, shp):
    return self.net.params[off:off + shp[0] * shp[1]].data_ptr()

  def _b(self, off):
    return self.net.params[off:].data_ptr()

  def _reset_words(self, st):
    self.net.lib.odin_range_reset(self.range_words.data_ptr(), self.range_words.numel() // RANGE_WORDS, st)

  def encode(self, z: torch.Tensor, eps2: Optional[torch.Tensor], seed: int, analytic: int, free_bits: float, st):
    """z -> encoder2 -> Latents2: p2, u = loc + softplus(raw) * eps2, kl2, fbmask"""
    lib, net, B = self.net.lib, self.net, self.B
    he = self.enc.forward(z, st)
    lib.odin_skip_head_fwd(z.data_ptr(), he.data_ptr(), self._w(net.lat_w_off, net.lat_shape), self._b(net.lat_b_off),
                           self.p2.data_ptr(), 0, None, None, None, None, B, net.D, net.He, 2 * net.Du, st)
    if eps2 is None:
      lib.odin_rng_normal(self.eps2.data_ptr(), B * net.Du, seed, self.hp(S2_STEP), st)
    elif eps2 is not self.eps2:
      self.eps2.copy_(eps2)
    lib.odin_latent_fwd(self.p2.data_ptr(), self.eps2.data_ptr(), self.u.data_ptr(), self.kl2.data_ptr(),
                        self.fbmask.data_ptr(), B, net.Du, analytic, free_bits, None, st)

  def decode(self, u: torch.Tensor, target: Optional[torch.Tensor], st):
    """u -> decoder2 -> Observation2: po; with a target also llk_raw = log p(target | u) and dpo = -d llk / d po / B"""
    lib, net, B = self.net.lib, self.net, self.B
    hd = self.dec.forward(u, st)
    if target is None:
      lib.odin_skip_head_fwd(u.data_ptr(), hd.data_ptr(), self._w(net.obs_w_off, net.obs_shape), self._b(net.obs_b_off),
                             self.po.data_ptr(), 0, None, None, None, None, B, net.Du, net.Hd, 2 * net.D, st)
    else:
      lib.odin_skip_head_fwd(u.data_ptr(), hd.data_ptr(), self._w(net.obs_w_off, net.obs_shape), self._b(net.obs_b_off),
                             self.po.data_ptr(), 1, target.data_ptr(), self.hp(S2_INVB), self.llk_raw.data_ptr(),
                             self.dpo.data_ptr(), B, net.Du, net.Hd, 2 * net.D, st)

  def sample_observation2(self, eps3: Optional[torch.Tensor], seed: int, st):
    """zs = a sample of q(z|u) = MVNDiag(po)"""
    lib, net, B = self.net.lib, self.net, self.B
    if eps3 is None:
      lib.odin_rng_normal(self.eps3.data_ptr(), B * net.D, seed, self.hp(S2_STEP), st)
    else:
      self.eps3.copy_(eps3)
    lib.odin_latent_fwd(self.po.data_ptr(), self.eps3.data_ptr(), self.zs.data_ptr(), self.kl_unused.data_ptr(),
                        self.mask_unused.data_ptr(), B, net.D, 0, -1.0, None, st)

  def forward(self, z, eps2, seed, analytic, free_bits, st, for_step: bool = False):
    """the stage-2 ELBO of z: llk [B], kl2 [B], out4 = (loss, mean llk, mean kl, 0)"""
    if self._words_dirty or not for_step:   # (a step's own reset rides in its slab reduction)
      self._reset_words(st)
    self._words_dirty = not for_step
    self.encode(z, eps2, seed, analytic, free_bits, st)
    self.decode(self.u, z, st)
    self.net.lib.odin_elbo_finalize(self.llk_raw.data_ptr(), 1, self.kl2.data_ptr(), self.hp(S2_BETA), None,
                                    self.llk.data_ptr(), self.out4.data_ptr(), self.B, st)

  def backward(self, z, analytic, st):
    """gradients of out4[0] with respect to every stage-2 parameter -> net.grads (z is data: no gradient leaves)"""
    lib, net, B = self.net.lib, self.net, self.B
    act = ACT[net.act]
    ne, nd = len(net.enc_recs), len(net.dec_recs)
    orows, lrows = C.c_int(0), C.c_int(0)
    lib.odin_skip_head_bwd(self.u.data_ptr(), self.dec.outs[-1].data_ptr(), self._w(net.obs_w_off, net.obs_shape),
                           self.dpo.data_ptr(), act, self.dec.gouts[-1].data_ptr(), self.dec.word(nd - 1),
                           self.du_head.data_ptr(), self.obs_slab.data_ptr(), C.byref(orows), B, net.Du, net.Hd,
                           2 * net.D, st)
    jobs = self.dec.backward(self.u, self.dec.gouts[-1], st, dx_out=self.du_stack)
    lib.odin_latent_bwd(self.p2.data_ptr(), self.eps2.data_ptr(), self.u.data_ptr(), self.du_head.data_ptr(),
                        self.du_stack.data_ptr(), self.fbmask.data_ptr(), self.hp(S2_INVB), None, None,
                        self.dp2.data_ptr(), B, net.Du, analytic, st)
    lib.odin_skip_head_bwd(z.data_ptr(), self.enc.outs[-1].data_ptr(), self._w(net.lat_w_off, net.lat_shape),
                           self.dp2.data_ptr(), act, self.enc.gouts[-1].data_ptr(), self.enc.word(ne - 1), None,
                           self.lat_slab.data_ptr(), C.byref(lrows), B, net.D, net.He, 2 * net.Du, st)
    jobs += self.enc.backward(z, self.enc.gouts[-1], st)
    assert 0 < orows.value <= self.obs_slab.shape[0] and 0 < lrows.value <= self.lat_slab.shape[0]
    for slab, off, rows in ((self.obs_slab, net.obs_w_off, orows.value), (self.lat_slab, net.lat_w_off, lrows.value)):
      jobs.append(ReduceJob(slab.data_ptr(), net.grads[off:].data_ptr(), slab.shape[1], rows, slab.shape[1], 0))
    rw = self.range_words   # (zero the range words: a reduction over zero slab rows, as DiscPrograms.reset_job)
    jobs.append(ReduceJob(rw.data_ptr(), rw.data_ptr(), rw.numel(), 0, rw.numel(), 0))
    arr = (ReduceJob * len(jobs))(*jobs)
    self._keep = arr
    lib.odin_slab_reduce(arr, len(jobs), st)

  def adam(self, check_nan: bool, st):
    lib, net = self.net.lib, self.net
    if check_nan:   # the gradient norm is the NaN guard: a non-finite one leaves parameters and moments alone
      lib.odin_sumsq_adam_flat(net.params.data_ptr(), net.grads.data_ptr(), net.m.data_ptr(), net.v.data_ptr(),
                               net.params.numel(), self.hp(S2_ALPHA), self.ws.data_ptr(), self.gnorm2.data_ptr(), 0.0,
                               net.flag.data_ptr(), st)
    else:
      lib.odin_adam_step_flat(net.params.data_ptr(), net.grads.data_ptr(), net.m.data_ptr(), net.v.data_ptr(),
                              net.params.numel(), self.hp(S2_ALPHA), None, 0.0, None, st)


class TwoStageVAE(BetaVAE):
  """two_stage_vae.py:17-216 (Dai & Wipf 2019, "Diagnosing and Enhancing VAE Models"): a second VAE over the latents of
  the first.  Stage 1 is the BetaVAE it extends -- same engine, same launches.  Stage 2 freezes it: z is the cached sample
  of q(z|x), q(u|z) = Latents2(encoder2(z)), p(z|u) = Observation2(decoder2(u)), loss = -mean(log p(z|u) - KL(q(u|z) ||
  N(0, I))), beta not applied; it trains exactly the stage-2 variables with its own Adam (`stage2_optimizer`: None or a
  dict learning_rate / beta_1 / beta_2 / epsilon; default Adam(1e-4)).  (The reference marks the stage-2 layers
  non-trainable at construction and never undoes it, so as shipped nothing trains in stage 2: DESIGN 3.19.)
  Stage-2 noise: keywords `eps` (z), `eps2` (u), `eps3` (the sample of q(z|u)); otherwise drawn on the device from the
  model's seed and step.  Stage-2 steps are launched eagerly."""

  _tril_refusal = "the second stage models the sample of a diagonal Gaussian q(z|x) ('mvndiag' only)"
  _concrete_refusal = _tril_refusal
  _relaxedbern_refusal = _tril_refusal

  def __init__(self, stage2_units: Sequence[int] = (1024, 1024, 1024), stage2_zdim: Optional[int] = None,
               stage2_iter_ratio: int = 4, stage2_optimizer: Optional[dict] = None, activation: str = 'relu',
               initializer=None, auto_train_2stages: bool = True, name='TwoStageVAE', **kwargs):
    if activation not in ACT:
      raise ValueError(f'TwoStageVAE: activation={activation!r} is outside the HIP path (relu, elu, linear)')
    if initializer not in (None, 'glorot_uniform'):
      raise NotImplementedError(f'TwoStageVAE: initializer={initializer!r}; the HIP path draws the Keras default '
                                '(glorot_uniform, zero biases)')
    self.stage2_units = tuple(int(u) for u in stage2_units)
    self._stage2_zdim = None if stage2_zdim is None else int(stage2_zdim)
    self.stage2_iter_ratio = int(stage2_iter_ratio)
    self.stage2_optimizer = dict(learning_rate=1e-4, beta_1=0.9, beta_2=0.999, epsilon=1e-7)
    if stage2_optimizer is not None:
      unknown = set(stage2_optimizer) - set(self.stage2_optimizer)
      if unknown:
        raise ValueError(f'TwoStageVAE: stage2_optimizer keys {sorted(unknown)} (Adam: {sorted(self.stage2_optimizer)})')
      self.stage2_optimizer.update({k: float(v) for k, v in stage2_optimizer.items()})
    self.stage2_activation = activation
    self.auto_train_2stages = bool(auto_train_2stages)
    self._train_stage1 = self._eval_stage1 = True
    self._stage2_net: Optional[Stage2Network] = None
    super().__init__(name=name, **kwargs)
    Stage2Network.check_limits(self.zdim, self.stage2_zdim, self.stage2_units)

  @property
  def stage2_zdim(self) -> int:
    return self.zdim if self._stage2_zdim is None else self._stage2_zdim

  @property
  def stage2(self) -> Stage2Network:
    if self._stage2_net is None:
      eng = self._engine(1)
      self._stage2_net = Stage2Network(eng.lib, self.zdim, self.stage2_zdim, self.stage2_units, self.stage2_activation,
                                       self.device, self.seed)
      from .dist import broadcast_parameters
      broadcast_parameters(self._stage2_net.params, src=0)
    return self._stage2_net

  # ---- stages ----
  def set_train_stage(self, stage: int) -> 'TwoStageVAE':
    if stage not in (1, 2):
      raise ValueError(f'stage={stage!r} (1 | 2)')
    self._train_stage1 = stage == 1
    return self

  def set_eval_stage(self, stage: int) -> 'TwoStageVAE':
    if stage not in (1, 2):
      raise ValueError(f'stage={stage!r} (1 | 2)')
    self._eval_stage1 = stage == 1
    return self

  train_stage = property(lambda self: 1 if self._train_stage1 else 2)
  eval_stage = property(lambda self: 1 if self._eval_stage1 else 2)

  def _kl_form(self) -> Tuple[int, float]:
    """(odin_latent_fwd's `analytic`, its `free_bits`) of the model's ELBO configuration"""
    return (2 if not self.reverse else int(self.analytic)), (-1.0 if self.free_bits is None else float(self.free_bits))

  def _stage2_refusals(self):
    if self.n_samples != 1:
      raise NotImplementedError(f'TwoStageVAE stage 2 with sample_shape={self.sample_shape}: the second stage reads ONE '
                                'cached sample of q(z|x) per input (sample_shape=())')
    if self._world_size() > 1 or bool(getattr(self, 'force_dp', False)):
      raise NotImplementedError('TwoStageVAE stage 2 under data parallelism: its gradients are not all-reduced '
                                '(train the second stage on one GPU)')

  def _first_stage(self, x: torch.Tensor, eps) -> Tuple[VAEEngine, Stage2Programs]:
    """the frozen first stage: run_encoder leaves q(z|x) in eng.p and its sample in eng.z"""
    eng = self._engine(x.shape[0])
    eng.set_hyper(beta=self.beta, t=self._step, **self._hyper_extra())
    eng.run_encoder(x, None if eps is None else _as_tensor(eps, self.device).reshape(x.shape[0], -1))
    return eng, self.stage2.bind(x.shape[0])

  def _noise(self, e, B, D):
    return None if e is None else _as_tensor(e, self.device).reshape(B, D)

  # ---- forward API ----
  def encode(self, inputs, training=None, mask=None, only_encoding=False, eps=None, eps2=None, eps3=None, **kwargs):
    """two_stage_vae.py:135-159: at eval stage 2 q(z|u) with u ~ q(u|z), z ~ q(z|x)"""
    if only_encoding or self._eval_stage1:
      return super().encode(inputs, training=training, mask=mask, only_encoding=only_encoding, eps=eps, **kwargs)
    return self.encode_two_stages(inputs, training=training, mask=mask, eps=eps, eps2=eps2, eps3=eps3)[2]

  def encode_two_stages(self, inputs, training=None, mask=None, eps=None, eps2=None, eps3=None):
    """-> (q(z|x), q(u|z), q(z|u)), each with its cached sample (two_stage_vae.py:161-179)"""
    self._stage2_refusals()
    x = _as_tensor(inputs, self.device)
    B = x.shape[0]
    eng, s2 = self._first_stage(x, eps)
    qz_x = self._posterior(eng)
    st = s2.stream()
    s2.set_hyper(self._step)
    s2._reset_words(st)
    s2._words_dirty = True
    s2.encode(eng.z, self._noise(eps2, B, self.stage2_zdim), self.seed + 17, 0, -1.0, st)
    s2.decode(s2.u, None, st)
    s2.sample_observation2(self._noise(eps3, B, self.zdim), self.seed + 19, st)
    qu_z = MVNDiagPosterior(s2.p2.clone(), s2.u.clone(), self.stage2_zdim)
    qz_u = MVNDiagPosterior(s2.po.clone(), s2.zs.clone(), self.zdim)
    return qz_x, qu_z, qz_u

  def elbo_components2(self, inputs, training=None, mask=None, eps=None, eps2=None, **kwargs):
    """two_stage_vae.py:181-192: ({'llk_<latents>': log p(z|u) [B]}, {'kl_latents2': KL(q(u|z) || p(u)) [B]})"""
    self._stage2_refusals()
    x = _as_tensor(inputs, self.device)
    eng, s2 = self._first_stage(x, eps)
    analytic, free_bits = self._kl_form()
    s2.set_hyper(self._step)
    s2.forward(eng.z, self._noise(eps2, x.shape[0], self.stage2_zdim), self.seed + 17, analytic, free_bits, s2.stream())
    return {f'llk_{self.latents.name}': s2.llk.clone()}, {'kl_latents2': s2.kl2.clone()}

  def elbo_components(self, inputs, training=None, mask=None, eps=None, **kwargs):
    if self._train_stage1:
      return super().elbo_components(inputs, training=training, mask=mask, eps=eps, **kwargs)
    return self.elbo_components2(inputs, training=training, mask=mask, eps=eps, **kwargs)

  def sample_prior(self, n: int = 1, seed: int = 1, two_stage: bool = True) -> torch.Tensor:
    """two_stage_vae.py:99-107: u ~ N(0, I) -> decoder2 -> observation2 -> a sample [n, D]"""
    if not two_stage:
      return super().sample_prior(n, seed=seed)
    n = int(n)
    g = torch.Generator(device='cpu').manual_seed(int(seed))
    u = torch.randn(n, self.stage2_zdim, generator=g).to(self.device)
    eps3 = torch.randn(n, self.zdim, generator=g).to(self.device)
    s2 = self.stage2.bind(n)
    st = s2.stream()
    s2.set_hyper(self._step)
    s2._reset_words(st)
    s2._words_dirty = True
    s2.decode(u.contiguous(), None, st)
    s2.sample_observation2(eps3, 0, st)
    return s2.zs.clone()

  def sample_observation(self, n: int = 1, seed: int = 1, training=False, two_stage: bool = True, **kwargs):
    return self.decode(self.sample_prior(n, seed=seed, two_stage=two_stage), training=training)

  # ---- training ----
  def optimize(self, inputs, training: bool = True, optimizer=None, learning_rate=1e-4, clipnorm=None, clipvalue=None,
               global_clipnorm=None, skip_update_threshold=None, when_skip_update: int = 0,
               nan_gradients_policy: str = 'skip', allow_none_gradients=False, aggregate_gradients=False,
               track_gradients=False, eps=None, use_graph: bool = False, eps2=None):
    """Stage 1: VariationalAutoencoder.optimize.  Stage 2: the frozen first stage's run_encoder, then the stage-2 step
    under `stage2_optimizer` (`learning_rate` belongs to the first optimiser and is not read, as the reference's second
    fit drops it); -> (loss, {'llk_<latents>', 'kl_latents2'}).  The clipping policies are not offered in stage 2."""
    if self._train_stage1:
      return super().optimize(inputs, training=training, optimizer=optimizer, learning_rate=learning_rate,
                              clipnorm=clipnorm, clipvalue=clipvalue, global_clipnorm=global_clipnorm,
                              skip_update_threshold=skip_update_threshold, when_skip_update=when_skip_update,
                              nan_gradients_policy=nan_gradients_policy, allow_none_gradients=allow_none_gradients,
                              aggregate_gradients=aggregate_gradients, track_gradients=track_gradients, eps=eps,
                              use_graph=use_graph)
    if nan_gradients_policy not in ('stop', 'skip', 'raise', 'ignore', 'restore'):
      raise ValueError(f'nan_gradients_policy={nan_gradients_policy!r}')
    if any(a is not None for a in (clipnorm, clipvalue, global_clipnorm, skip_update_threshold)):
      raise NotImplementedError('TwoStageVAE stage 2: clipnorm / clipvalue / global_clipnorm / skip_update_threshold are '
                                'not wired to the second optimiser')
    self._stage2_refusals()
    x = _as_tensor(inputs, self.device)
    if training:
      self._step += 1
    eng, s2 = self._first_stage(x, eps)
    net = s2.net
    analytic, free_bits = self._kl_form()
    st = s2.stream()
    s2.set_hyper(self._step, self.stage2_optimizer if training else None)
    s2.forward(eng.z, self._noise(eps2, x.shape[0], self.stage2_zdim), self.seed + 17, analytic, free_bits, st,
               for_step=training)
    if training:
      s2.backward(eng.z, analytic, st)
      s2.adam(nan_gradients_policy != 'ignore', st)
      net.t += 1
    out = s2.out4.clone()
    metrics = {f'llk_{self.latents.name}': out[1], 'kl_latents2': out[2]}
    if training and track_gradients:
      for (name, off, shp) in net.names():
        metrics['_grad/' + name] = net.grads[off:off + int(np.prod(shp))].view(shp).clone()
    return out[0], metrics

  @property
  def nan_flag(self) -> bool:
    s2 = self._stage2_net
    return super().nan_flag or (s2 is not None and int(s2.flag.item()) != 0)

  def _nan_flags(self, eng) -> List[torch.Tensor]:
    return [eng.flag] if (self._train_stage1 or self._stage2_net is None) else [self._stage2_net.flag]

  def fit(self, train, *, valid=None, **kwargs):
    """two_stage_vae.py:202-216: the normal fit; then, still in stage 1 and `auto_train_2stages`, stage 2 for
    stage2_iter_ratio x the requested max_iter / epochs under the second optimiser, and back to stage 1"""
    super().fit(train, valid=valid, **kwargs)
    if self._train_stage1 and self.auto_train_2stages:
      self.set_train_stage(2)
      try:
        for k in ('on_batch_end', 'on_valid_end', 'optimizer', 'learning_rate'):
          kwargs.pop(k, None)
        super().fit(train, epochs=kwargs.pop('epochs', -1) * self.stage2_iter_ratio,
                    max_iter=kwargs.pop('max_iter', 1000) * self.stage2_iter_ratio, **kwargs)
      finally:
        self.set_train_stage(1)
    return self

  # ---- checkpoints: the four stage-2 layers and the second optimiser are attributes of the reference's model ----
  def _extra_checkpoint_variables(self) -> Dict[str, np.ndarray]:
    net = self.stage2
    W = {}
    for name, off, shp in net.names():
      n = int(np.prod(shp))
      W[name] = net.params[off:off + n].view(shp).detach().cpu().numpy()
      W[f'stage2_optimizer/{name}/m'] = net.m[off:off + n].view(shp).detach().cpu().numpy()
      W[f'stage2_optimizer/{name}/v'] = net.v[off:off + n].view(shp).detach().cpu().numpy()
    W['stage2_optimizer/iter'] = np.asarray(net.t, np.int64)
    return W

  def _load_extra_checkpoint_variables(self, d: Dict[str, np.ndarray]):
    net = self.stage2
    names = net.names()
    if not any(n == nm or n.endswith('/' + nm) for n in d for nm, _, _ in names):
      return   # a checkpoint of the first stage alone (a BetaVAE's): the second stage keeps what it holds
    as_t = lambda a: torch.as_tensor(np.asarray(a), dtype=torch.float32, device=self.device)
    for name, off, shp in names:
      n = int(np.prod(shp))
      a = self._find_variable(d, name)
      if tuple(a.shape) != tuple(shp):
        raise ValueError(f'{name}: checkpoint shape {a.shape} != {tuple(shp)}')
      net.params[off:off + n].view(shp).copy_(as_t(a))
      for slot, buf in (('m', net.m), ('v', net.v)):
        buf[off:off + n].view(shp).copy_(as_t(self._find_variable(d, f'stage2_optimizer/{name}/{slot}')))
    net.t = int(self._find_variable(d, 'stage2_optimizer/iter'))


# ======================================================================================
# MultitaskVAE / SkiptaskVAE: semi-supervised label head on the latents (multitask_vae.py)
# ======================================================================================
class OneHotCategoricalLabels:
  """OneHotCategorical(logits) as predict_labels returns it: what callers of the reference read from p(y|z)."""

  def __init__(self, logits: torch.Tensor):
    self.logits = logits
    self.event_shape = (int(logits.shape[-1]),)
    self.batch_shape = tuple(logits.shape[:-1])

  def probs_parameter(self) -> torch.Tensor:
    return torch.softmax(self.logits, -1)

  def mean(self) -> torch.Tensor:
    return self.probs_parameter()

  def mode(self) -> torch.Tensor:
    """one-hot rows at the largest logit (the class index: mode().argmax(-1))"""
    return torch.nn.functional.one_hot(self.logits.argmax(-1), self.logits.shape[-1]).to(self.logits.dtype)

  def log_prob(self, y) -> torch.Tensor:
    """sum_k y_k log_softmax(logits)_k (TFP's OneHotCategorical._log_prob: soft labels too)"""
    y = torch.as_tensor(y, dtype=self.logits.dtype, device=self.logits.device)
    return (y * torch.log_softmax(self.logits, -1)).sum(-1)

  def sample(self, n=None, seed=None) -> torch.Tensor:
    g = None if seed is None else torch.Generator(device='cpu').manual_seed(int(seed))   # (None: torch's own stream)
    pr = self.probs_parameter().reshape(-1, self.logits.shape[-1]).cpu()
    idx = torch.multinomial(pr, int(n or 1), replacement=True, generator=g).T   # [n, rows]
    oh = torch.nn.functional.one_hot(idx, self.logits.shape[-1]).to(dtype=self.logits.dtype, device=self.logits.device)
    oh = oh.reshape((int(n or 1),) + tuple(self.logits.shape))
    return oh[0] if n is None else oh


class MultitaskVAE(AnnealingVAE):
  """multitask_vae.py:21-207 (Trong et al. 2019): an AnnealingVAE with labels = RVconf(K, 'onehot', projection=True), a
  Dense(zdim -> K) on a FRESH sample z' of q(z|x) giving the logits of p(y|z').  Inputs are x, (x,) or
  (x_u, x_s, y_s) with equal halves; a labelled call evaluates
    loss = -mean_u(llk_u - kl_u) - mean_s(llk_s - kl_s) - alpha * mean_s log p(y_s | z')
  (the two half-batch means added) as ONE engine step over cat(x_u, x_s).  Built is the form that reads the latents
  directly (skip_decoder=True, SkiptaskVAE): here the decoder's last layer is the observation's own projection."""

  _tril_refusal = "the label head's fresh sample is written for the 'mvndiag' posterior"
  _concrete_refusal = _tril_refusal
  _relaxedbern_refusal = _tril_refusal

  def __init__(self, labels: RVconf = None, encoder_y=None, decoder_y=None, alpha: float = 10., n_semi_iw=(),
               skip_decoder: bool = False, name: str = 'MultitaskVAE', **kwargs):
    if labels is None:
      labels = RVconf(10, 'onehot', projection=True, name='digits')
    if isinstance(labels, (list, tuple)):
      raise NotImplementedError('a list of label variables: the label head is ONE OneHotCategorical over the latents')
    if not isinstance(labels, RVconf):
      raise ValueError(f'labels must be an RVconf, got {type(labels)}')
    if str(labels.posterior).lower() not in ('onehot', 'onehotcategorical'):
      raise NotImplementedError(f"labels posterior {labels.posterior!r}: the label kernel evaluates 'onehot' "
                                f'(OneHotCategorical) only')
    if len(tuple(labels.event_shape)) != 1 or not labels.projection:
      raise NotImplementedError("labels must be RVconf(K, 'onehot', projection=True): one K-way variable behind a Dense "
                                'projection of the latents')
    if not skip_decoder:
      raise NotImplementedError("skip_decoder=False: the decoder's last layer is the observation's projection here, so "
                                'there is no decoder activation h_d for the labels to read; use SkiptaskVAE')
    if encoder_y is not None:
      raise NotImplementedError("encoder_y: a second posterior q(z_y|x) ('tie' / 'copy' / a network) is not built")
    if decoder_y is not None:
      raise NotImplementedError('decoder_y: hidden layers between the latents and the labels are not built (MultiheadVAE '
                                'would add a batch-normalised stack, and the engine has no batch normalisation)')
    if isinstance(n_semi_iw, (int, np.integer)) and not isinstance(n_semi_iw, bool):
      raise NotImplementedError(f'n_semi_iw={n_semi_iw}: importance-weighted label samples are not built (n_semi_iw=() '
                                f'draws the one fresh sample)')
    if tuple(n_semi_iw) != ():
      raise NotImplementedError(f'n_semi_iw={n_semi_iw!r}: only () is built')
    ss = kwargs.get('sample_shape', ())
    if (ss if isinstance(ss, int) else tuple(ss)) != ():
      raise NotImplementedError(f'sample_shape={ss!r}: a labelled step lays the batch out as cat(x_u, x_s), the tiled '
                                f'batch of sample_shape would break the halves apart')
    self.labels, self.alpha = labels, float(alpha)
    self.n_semi_iw, self.skip_decoder, self.encoder_y, self.decoder_y = (), True, None, None
    super().__init__(name=name, **kwargs)

  def _reg_options(self) -> dict:
    return dict(label_units=int(self.labels.event_size))

  def set_elbo_configs(self, analytic=None, reverse=None, free_bits=None, sample_shape=None):
    if sample_shape is not None and (sample_shape if isinstance(sample_shape, int) else tuple(sample_shape)) != ():
      raise NotImplementedError(f'sample_shape={sample_shape!r} is not offered by {type(self).__name__}')
    return super().set_elbo_configs(analytic=analytic, reverse=reverse, free_bits=free_bits)

  def variable_name(self, key: tuple) -> str:
    if key[0] == 'lab':
      return f"{self.labels.name}/{'kernel' if key[-1] == 'w' else 'bias'}"
    return super().variable_name(key)

  # ---- inputs -----------------------------------------------------------------------------------------------------------
  def _ssl_inputs(self, inputs):
    """x | (x,) | (x_u, x_s, y_s) -> (x_u, x_s or None, y_s [B_s, K] float or None)"""
    if not isinstance(inputs, (tuple, list)):
      return _as_tensor(inputs, self.device), None, None
    if len(inputs) == 1:
      return _as_tensor(inputs[0], self.device), None, None
    if len(inputs) != 3:
      raise ValueError(f'inputs must be x, (x,) or (x_u, x_s, y_s): got {len(inputs)} elements')
    x_u, x_s = _as_tensor(inputs[0], self.device), _as_tensor(inputs[1], self.device)
    K = int(self.labels.event_size)
    y = inputs[2]
    y = y if torch.is_tensor(y) else torch.as_tensor(np.asarray(y))
    if y.dim() == 1:   # integer classes
      if y.is_floating_point() and bool((y != y.round()).any()):
        raise ValueError('labels of one axis must be integer classes')
      y = y.to(torch.int64)
      if bool(((y < 0) | (y >= K)).any()):
        raise ValueError(f'integer labels outside [0, {K})')
      y = torch.nn.functional.one_hot(y, K)
    y = y.to(device=self.device, dtype=torch.float32).contiguous()
    if x_u.shape[0] != x_s.shape[0]:
      raise ValueError(f'a labelled step needs equal halves: {x_u.shape[0]} unlabelled and {x_s.shape[0]} labelled rows')
    if tuple(y.shape) != (x_s.shape[0], K):
      raise ValueError(f'labels: expected [{x_s.shape[0]}, {K}] or [{x_s.shape[0]}], got {tuple(y.shape)}')
    return x_u, x_s, y

  def _names(self):
    o, l, y = self.observation.name, self.latents.name, self.labels.name
    return f'uns/llk_{o}', f'uns/kl_{l}', f'sup/llk_{o}', f'sup/kl_{l}', f'sup/llk_{y}'

  def _fit_batch(self, b):
    if not isinstance(b, (tuple, list)):
      return _as_tensor(b, self.device)
    t = self._ssl_inputs(b)
    return t[0] if t[1] is None else t

  def _fit_batch_rows(self, xb) -> int:
    return 2 * xb[0].shape[0] if isinstance(xb, tuple) else xb.shape[0]

  # ---- forward API ------------------------------------------------------------------------------------------------------
  def encode(self, inputs, training=None, mask=None, only_encoding=False, eps=None, **kwargs):
    """the labels are never conditioned on: the first (unlabelled) input is encoded (multitask_vae.py:129-142)"""
    return super().encode(self._ssl_inputs(inputs)[0], training=training, mask=mask, only_encoding=only_encoding,
                          eps=eps)

  def predict_labels(self, inputs=None, latents=None, training=None, mask=None, n_mcmc=(), mean=False, seed=None,
                     **kwargs) -> OneHotCategoricalLabels:
    """multitask_vae.py:95-127 with skip_decoder=True: p(y|z) at the posterior's mean (`mean=True`) or at a fresh sample
    of it; `latents` may be a posterior or a tensor of codes [n, zdim].  classify: predict_labels(x, mean=True).mode()"""
    if n_mcmc != ():
      raise NotImplementedError(f'n_mcmc={n_mcmc!r}: only the single sample () is built')
    if latents is None:
      latents = self.encode(inputs, training=training, mask=mask)
    if isinstance(latents, MVNDiagPosterior):
      z = latents.mean() if mean else latents.sample(seed=seed)
    else:
      z = latents
    z = _as_tensor(z, self.device).reshape(-1, self.zdim)
    # (the launch takes any number of rows and needs no per-batch plan: the engine build() made serves)
    return OneHotCategoricalLabels(self._engine(1).label_logits(z))

  def call(self, inputs, training=None, mask=None, eps=None, **kwargs):
    """-> ((p(x|z), p(y|z)), q(z|x)) (multitask_vae.py:144-156)"""
    qz_x = self.encode(inputs, training=training, mask=mask, eps=eps)
    py_z = self.predict_labels(latents=qz_x, training=training, mask=mask)
    px_z = self.decode(qz_x, training=training, mask=mask)
    self._last_outputs = ((px_z, py_z), qz_x)
    return (px_z, py_z), qz_x

  __call__ = call

  def _labelled_forward(self, x_u, x_s, y, eps, eps_y):
    x = torch.cat([x_u, x_s]).contiguous()
    eng = self._engine(x.shape[0])
    eng.set_labels(y, None if eps_y is None else _as_tensor(eps_y, self.device))
    eng.set_hyper(beta=self.beta, t=self._step, label_alpha=self.alpha, **self._hyper_extra())
    eng.forward(x, None if eps is None else _as_tensor(eps, self.device).reshape(x.shape[0], -1))
    return eng

  def elbo_components(self, inputs, training=None, mask=None, eps=None, eps_y=None, **kwargs):
    """multitask_vae.py:164-207 + merge_objectives (variational_autoencoder.py:622-632): the unlabelled entries per
    sample, the labelled ones reduced to scalars; llk['sup/llk_<labels>'] = alpha * mean_s log p(y_s | z')"""
    x_u, x_s, y = self._ssl_inputs(inputs)
    n = self._names()
    if x_s is None:
      self._engine(x_u.shape[0]).set_labels(None)
      llk, kl = super().elbo_components(x_u, training=training, mask=mask, eps=eps)
      return {'uns/' + k: v for k, v in llk.items()}, {'uns/' + k: v for k, v in kl.items()}
    eng = self._labelled_forward(x_u, x_s, y, eps, eps_y)
    h = x_u.shape[0]
    qz_x = MVNDiagPosterior(eng.p[h:].clone(), eng.z[h:].clone(), eng.D)
    self._last_outputs = ((self._observation_dist(eng.dec.outs[-1][h:].clone()),
                           OneHotCategoricalLabels(eng.lab_logits.clone())), qz_x)
    klv = eng.kl.clone() * self.beta
    llk = {n[0]: eng.llk[:h].clone(), n[2]: eng.llk[h:].mean(), n[4]: -eng.out4[3].clone()}
    kl = {n[1]: klv[:h].unsqueeze(0) if self.analytic else klv[:h], n[3]: klv[h:].mean()}
    return llk, kl

  def optimize(self, inputs, training: bool = True, optimizer=None, learning_rate=1e-4,
               clipnorm=None, clipvalue=None, global_clipnorm=None, skip_update_threshold=None,
               when_skip_update: int = 0, nan_gradients_policy: str = 'skip',
               allow_none_gradients=False, aggregate_gradients=False, track_gradients=False,
               eps=None, use_graph: bool = False, eps_y=None):
    """Networks.optimize over x, (x,) or (x_u, x_s, y_s).  An unlabelled call is the AnnealingVAE step (the label
    variables receive a zero gradient); a labelled one runs cat(x_u, x_s) as one engine step whose gradient is the
    reference's, so every gradient policy acts on it.  `eps` [B_u + B_s, zdim] / `eps_y` [B_s, zdim] fix the noise of z
    and of the fresh sample z' (tests)."""
    x_u, x_s, y = self._ssl_inputs(inputs)
    n = self._names()
    if x_s is None:
      assert eps_y is None, 'eps_y belongs to a labelled step'
      self._engine(x_u.shape[0]).set_labels(None)
      loss, m = super().optimize(x_u, training=training, learning_rate=learning_rate, clipnorm=clipnorm,
                                 clipvalue=clipvalue, global_clipnorm=global_clipnorm,
                                 skip_update_threshold=skip_update_threshold, when_skip_update=when_skip_update,
                                 nan_gradients_policy=nan_gradients_policy, track_gradients=track_gradients, eps=eps,
                                 use_graph=use_graph)
      ren = {f'llk_{self.observation.name}': n[0], f'kl_{self.latents.name}': n[1]}
      return loss, {ren.get(k, k): v for k, v in m.items()}
    if nan_gradients_policy not in ('stop', 'skip', 'raise', 'ignore', 'restore'):
      raise ValueError(f'nan_gradients_policy={nan_gradients_policy!r}')
    x = torch.cat([x_u, x_s]).contiguous()
    eng = self._engine(x.shape[0])
    if eps is not None:
      eps = _as_tensor(eps, self.device).reshape(x.shape[0], -1)
    if eps_y is not None:
      eps_y = _as_tensor(eps_y, self.device).reshape(x_s.shape[0], -1)
    if training:
      self._step += 1
    eng.step_count = self._step - 1 if training else self._step
    if not training:
      eng.set_labels(y, eps_y)
      eng.set_hyper(beta=self.beta, t=self._step, label_alpha=self.alpha, **self._hyper_extra())
      eng.forward(x, eps)
    else:
      eng.train_step(x, eps, lr=self._lr(learning_rate), beta=self.beta, global_clipnorm=global_clipnorm,
                     use_graph=use_graph, clipnorm=clipnorm, clipvalue=clipvalue,
                     skip_update_threshold=skip_update_threshold, when_skip_update=when_skip_update,
                     check_nan=nan_gradients_policy != 'ignore', labels=y, eps_y=eps_y, label_alpha=self.alpha,
                     **self._hyper_extra())
      self._step = eng.step_count
    o = eng.label_step_outputs(self.beta)
    metrics = {n[0]: o['uns/llk'], n[1]: o['uns/kl'], n[2]: o['sup/llk'], n[3]: o['sup/kl'], n[4]: o['sup/llk_y']}
    if training and track_gradients:
      for k, g in eng.grad_views().items():
        metrics['_grad/' + self.variable_name(k)] = g.clone()
    return o['loss'], metrics

  # ---- checkpoints: the label variables travel with every other parameter; their Adam slots beside them -------------------
  def _label_slots(self):
    eng = self._engine(1)
    for key, shp, off in eng.layout.entries:
      if key[0] == 'lab':
        n = int(np.prod(shp))
        yield f'optimizer/{self.variable_name(key)}', eng.m[off:off + n].view(shp), eng.v[off:off + n].view(shp)

  def _extra_checkpoint_variables(self) -> Dict[str, np.ndarray]:
    W = {}
    for name, m, v in self._label_slots():
      W[f'{name}/m'] = m.detach().cpu().numpy()
      W[f'{name}/v'] = v.detach().cpu().numpy()
    return W

  def _load_extra_checkpoint_variables(self, d: Dict[str, np.ndarray]):
    for name, m, v in self._label_slots():
      for slot, dst in (('m', m), ('v', v)):
        nm = f'{name}/{slot}'
        if nm in d or any(k.endswith('/' + nm) for k in d):   # (a checkpoint without the slots: they stay as they are)
          dst.copy_(torch.as_tensor(np.asarray(self._find_variable(d, nm)), dtype=torch.float32, device=self.device))


class SkiptaskVAE(MultitaskVAE):
  """multitask_vae.py:226-240: the labels read the latents directly (skip_decoder=True, no decoder_y)"""

  def __init__(self, encoder_y=None, name: str = 'SkiptaskVAE', **kwargs):
    kwargs.pop('skip_decoder', None)
    kwargs.pop('decoder_y', None)
    super().__init__(encoder_y=encoder_y, decoder_y=None, skip_decoder=True, name=name, **kwargs)


class MultiheadVAE(MultitaskVAE):
  """multitask_vae.py:243-264: refused -- its decoder_y is a batch-normalised Dense stack, and the engine has no batch
  normalisation"""

  def __init__(self, decoder_y=None, name: str = 'MultiheadVAE', **kwargs):
    raise NotImplementedError('MultiheadVAE: its decoder_y is a batch-normalised Dense stack (NetConf((512, 512), '
                              'batchnorm=True)); the engine has no batch normalisation -- use SkiptaskVAE')


def get_vae(name: str):
  """odin/bay/vi/autoencoder/__init__.py:28"""
  table = {c.__name__.lower(): c for c in (VariationalAutoencoder, BetaVAE, AnnealingVAE,
                                           BetaTCVAE, FactorVAE, BetaCapacityVAE, InfoVAE, DIPVAE,
                                           VampriorVAE, VQVAE, TwoStageVAE, MultitaskVAE, SkiptaskVAE)}
  table['vae'] = VariationalAutoencoder
  key = str(name).lower().replace('_', '')
  if key not in table:
    raise ValueError(f'Cannot find VAE {name!r}; the HIP path offers {sorted(table)}')
  return table[key]
