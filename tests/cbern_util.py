"""Float64 restatement of the continuous Bernoulli observation ('cbernoulli'; Loaiza-Ganem & Cunningham 2019) in logit
space, the reference of tests/test_cbernoulli.py.  For a logit l and a target x in [0, 1]:

  log p(x | l) = x l - A(l),  A(l) = log((e^l - 1) / l),  A(0) = 0
  mu(l) = A'(l) = 1 / (1 - e^-l) - 1 / l,  mu(0) = 1/2

A and mu come from their series below |l| < SERIES_BELOW (nine terms: the truncation at 1e-2 is below 1e-40) and from the
closed forms above; `*_series` and `*_closed` are exported so that the test can compare them where both are accurate.  The
CDF and its inverse are written with expm1 / log1p, which are exact to rounding at every l != 0 (at l = 0 the
distribution is uniform): they need no series.  Everything takes and returns float64 torch tensors, so autograd runs
through it (the training-step reference)."""
import math

import numpy as np
import torch

F64 = torch.float64
SERIES_BELOW = 1e-2

# Bernoulli numbers B_2k, k = 1 .. 9:  A(l) = l/2 + sum B_2k l^2k / (2k (2k)!),  mu(l) = 1/2 + sum B_2k l^(2k-1) / (2k)!
_B2K = [1 / 6, -1 / 30, 1 / 42, -1 / 30, 5 / 66, -691 / 2730, 7 / 6, -3617 / 510, 43867 / 798]


def t64(a):
  return torch.as_tensor(np.asarray(a, dtype=np.float64), dtype=F64) if not torch.is_tensor(a) else a.to(F64)


def log_norm_series(l):
  s = 0.5 * l
  for k, b in enumerate(_B2K, 1):
    s = s + b * l ** (2 * k) / (2 * k * math.factorial(2 * k))
  return s


def mean_series(l):
  s = 0.5 + 0.0 * l
  for k, b in enumerate(_B2K, 1):
    s = s + b * l ** (2 * k - 1) / math.factorial(2 * k)
  return s


def log_norm_closed(l):
  """A(l) for l != 0: |l| + log1p(-e^-|l|) - log |l|, minus |l| for a negative l"""
  a = l.abs()
  return torch.clamp(l, min=0.0) + torch.log1p(-torch.exp(-a)) - torch.log(a)


def mean_closed(l):
  """mu(l) for l != 0: 1 / (1 - e^-|l|) - 1 / |l| on the positive side, one minus it on the negative side"""
  a = l.abs()
  m = -1.0 / torch.expm1(-a) - 1.0 / a
  return torch.where(l >= 0, m, 1.0 - m)


def _pick(l, series, closed):
  small = l.abs() < SERIES_BELOW
  safe = torch.where(small, torch.ones_like(l), l)
  return torch.where(small, series(l), closed(safe))


def log_norm(l):
  return _pick(l, log_norm_series, log_norm_closed)


def mean(l):
  return _pick(l, mean_series, mean_closed)


def log_prob(l, x):
  """elementwise log p(x | l)"""
  return x * l - log_norm(l)


def log_prob_sum(l, x):
  """per sample: the sum over everything but the leading axis"""
  e = log_prob(l, x)
  return e.reshape(e.shape[0], -1).sum(1)


def cdf(l, x):
  """F(x) = (e^(l x) - 1) / (e^l - 1); x at l = 0"""
  zero = l == 0
  safe = torch.where(zero, torch.ones_like(l), l)
  return torch.where(zero, x, torch.expm1(safe * x) / torch.expm1(safe))


def icdf(l, u):
  """l > 0: 1 + log(u + (1 - u) e^-l) / l = 1 + log1p((1 - u) expm1(-l)) / l;  l < 0: 1 - icdf(-l, 1 - u);  l = 0: u"""
  zero = l == 0
  a = torch.where(zero, torch.ones_like(l), l.abs())
  v = torch.where(l >= 0, u, 1.0 - u)
  y = 1.0 + torch.log1p((1.0 - v) * torch.expm1(-a)) / a
  return torch.where(zero, u, torch.where(l >= 0, y, 1.0 - y))


def np_log_prob_sum(l, x):
  return log_prob_sum(t64(l), t64(x)).numpy()


def np_mean(l):
  return mean(t64(l)).numpy()


class CBernRef:
  """The training step of a Gaussian-latent VAE with the continuous Bernoulli observation, float64 autograd through
  oracle.torch_ref.t_seq: loss = -mean(llk - beta * kl) with the single-sample KL."""

  def __init__(self, enc, dec, zdim, beta):
    self.enc, self.dec, self.D, self.beta = list(enc), list(dec), int(zdim), float(beta)

  def loss_and_grads(self, P, x, eps):
    from oracle.torch_ref import TorchVAE, t_seq
    T = {k: torch.tensor(np.asarray(v), dtype=F64, requires_grad=True) for k, v in P.items()}
    xt, et = t64(x), t64(eps)
    D = self.D
    h_e = t_seq(self.enc, TorchVAE._sub(T, 'enc'), xt)
    p = h_e @ T[('lat', 'w')] + T[('lat', 'b')]
    loc, scale = p[:, :D], torch.nn.functional.softplus(p[:, D:])
    z = loc + scale * et
    h_d = t_seq(self.dec, TorchVAE._sub(T, 'dec'), z)
    llk = log_prob_sum(h_d, xt)
    kl = (0.5 * (z ** 2 - et ** 2) - torch.log(scale)).sum(-1)
    loss = -(llk - self.beta * kl).mean()
    loss.backward()
    G = {k: v.grad.detach().numpy() for k, v in T.items()}
    f = dict(h_d=h_d.detach().numpy(), llk=llk.detach().numpy(), kl=kl.detach().numpy(), loss=float(loss.detach()))
    return f, G
