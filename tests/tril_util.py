"""float64 restatement of the full-covariance Gaussian posterior 'mvntril' (tests only).

Source of truth: MultivariateNormalLayer.new with covariance='tril' (odin/bay/layers/continuous.py:459-474) and TFP's
documented FillScaleTriL(diag_bijector=softplus, diag_shift=1e-5) -> FillTriangular: the D (D + 1) / 2 raw values r are
laid out as `concat(r[D:], reverse(r))` read row-major as a D x D matrix of which the lower triangle is kept
(FillTriangular([1, 2, 3, 4, 5, 6]) = [[4, 0, 0], [6, 5, 0], [3, 2, 1]]).  TFP is not available here: parity with the
reference is unpinned, like the rest of the VAE oracle.

Everything is torch float64 so that autograd can check the hand-written gradients; the hand gradients below are derived
from the formulas of this file, in matrix form -- not from the kernel.
"""
import math

import numpy as np
import torch

LOG2PI = math.log(2.0 * math.pi)
DIAG_SHIFT = 1e-5


def n_tril(D):
  return D * (D + 1) // 2


def fill_index(i, j, D):
  """index into r of L_raw[i][j], j <= i -- the closed form the kernels use"""
  k, M = i * D + j, n_tril(D)
  return D + k if k < M - D else D * D - 1 - k


def fill_triangular(r, D):
  """TFP's FillTriangular (upper=False) by its documented construction; r [..., M] -> [..., D, D]"""
  x = torch.cat([r[..., D:], torch.flip(r, dims=(-1,))], -1)
  return torch.tril(x.reshape(tuple(r.shape[:-1]) + (D, D)))


def softplus(x):
  return torch.logaddexp(x, torch.zeros_like(x))


def split(p, D):
  """p [..., D + M] -> loc [..., D], raw L [..., D, D] (lower triangle of r), L = scale_tril [..., D, D]"""
  p = torch.as_tensor(p, dtype=torch.float64) if not torch.is_tensor(p) else p
  loc, r = p[..., :D], p[..., D:]
  Lr = fill_triangular(r, D)
  d = softplus(torch.diagonal(Lr, dim1=-2, dim2=-1)) + DIAG_SHIFT
  return loc, Lr, torch.tril(Lr, -1) + torch.diag_embed(d)


def sample(loc, L, eps):
  return loc + (L @ eps[..., None])[..., 0]


def log_q(L, eps):
  """log q(z) at z = loc + L eps"""
  D = L.shape[-1]
  return -0.5 * (eps ** 2).sum(-1) - torch.log(torch.diagonal(L, dim1=-2, dim2=-1)).sum(-1) - 0.5 * D * LOG2PI


def log_p(z):
  return -0.5 * (z ** 2).sum(-1) - 0.5 * z.shape[-1] * LOG2PI


def kl_mc(loc, L, eps):
  return log_q(L, eps) - log_p(sample(loc, L, eps))


def kl_closed(loc, L):
  D = L.shape[-1]
  return 0.5 * ((L ** 2).sum((-2, -1)) + (loc ** 2).sum(-1) - D) - torch.log(torch.diagonal(L, dim1=-2, dim2=-1)).sum(-1)


def clamp(kl, D, free_bits=None, capacity=None):
  """-> (kl after free bits / capacity, fbmask): max(kl, free_bits D), then |kl - C| with the sign in the mask"""
  m = torch.ones_like(kl)
  if free_bits is not None:
    thr = free_bits * D
    hit = ~(kl > thr)
    m = torch.where(hit, torch.zeros_like(m), m)
    kl = torch.where(hit, torch.full_like(kl, thr), kl)
  if capacity is not None:
    d = kl - capacity
    m = m * torch.sign(d)
    kl = d.abs()
  return kl, m


def latent_fwd(p, eps, D, analytic, free_bits=None, capacity=None):
  """-> z, kl (after the clamps), fbmask, kl before the clamps"""
  p, eps = (torch.as_tensor(np.asarray(a), dtype=torch.float64) if not torch.is_tensor(a) else a for a in (p, eps))
  loc, _, L = split(p, D)
  raw_kl = kl_closed(loc, L) if analytic else kl_mc(loc, L, eps)
  kl, m = clamp(raw_kl, D, free_bits, capacity)
  return sample(loc, L, eps), kl, m, raw_kl


def latent_bwd(p, eps, g, fbmask, klw, D, analytic):
  """dp [B, D + M] of  sum_b (klw fbmask_b kl_b + g_b . z_b)  by hand.
  z = loc + L eps: dz/dloc = I, dz/dL_ij = eps_j e_i.  MC: kl = -1/2 |eps|^2 - sum log L_ii + 1/2 |z|^2 + const, so
  dkl/dz = z and dkl/dL_ii gets -1 / L_ii; closed form: dkl/dloc = loc, dkl/dL = L - diag(1 / L_ii)."""
  p, eps, g, fbmask = (torch.as_tensor(np.asarray(a), dtype=torch.float64) for a in (p, eps, g, fbmask))
  loc, Lr, L = split(p, D)
  w = (klw * fbmask)[:, None]
  inv_d = torch.diag_embed(1.0 / torch.diagonal(L, dim1=-2, dim2=-1))
  if analytic:
    dloc = g + w * loc
    dL = g[:, :, None] * eps[:, None, :] + w[:, :, None] * (L - inv_d)
  else:
    gz = g + w * sample(loc, L, eps)
    dloc = gz
    dL = gz[:, :, None] * eps[:, None, :] - w[:, :, None] * inv_d
  # through the fill: the diagonal passes softplus (derivative sigmoid of the raw value), the rest is the identity
  sig = torch.sigmoid(torch.diagonal(Lr, dim1=-2, dim2=-1))
  dLr = torch.tril(dL, -1) + torch.diag_embed(torch.diagonal(dL, dim1=-2, dim2=-1) * sig)
  M = n_tril(D)
  dr = torch.zeros(p.shape[0], M, dtype=torch.float64)
  for i in range(D):
    for j in range(i + 1):
      dr[:, fill_index(i, j, D)] = dLr[:, i, j]
  return torch.cat([dloc, dr], -1)


def t_mmd(x, y):
  D = x.shape[1]

  def k(a, b):
    return torch.exp(-((a[:, None, :] - b[None, :, :]) ** 2).sum(-1) / D)
  return k(x, x).mean() + k(y, y).mean() - 2.0 * k(x, y).mean()


class TrilRef:
  """The whole step in torch float64 autograd over oracle.torch_ref's layers: encoder -> Dense(D + M) -> mvntril
  posterior -> decoder -> Bernoulli log-likelihood; loss = -mean llk + beta mean kl (+ reg_coef MMD(z, y))."""

  def __init__(self, enc, dec, zdim, analytic=False, beta=1.0, free_bits=None, reg_coef=None):
    self.enc, self.dec, self.D = list(enc), list(dec), int(zdim)
    self.analytic, self.beta, self.free_bits, self.reg_coef = bool(analytic), float(beta), free_bits, reg_coef

  def forward(self, T, x, eps, prior=None):
    from oracle.torch_ref import TorchVAE, t_seq
    D, B = self.D, x.shape[0]
    h_e = t_seq(self.enc, TorchVAE._sub(T, 'enc'), x)
    p = h_e @ T[('lat', 'w')] + T[('lat', 'b')]
    loc, _, L = split(p, D)
    z = sample(loc, L, eps)
    h_d = t_seq(self.dec, TorchVAE._sub(T, 'dec'), z)
    llk = (x * h_d - softplus(h_d)).reshape(B, -1).sum(1)
    kl, _ = clamp(kl_closed(loc, L) if self.analytic else kl_mc(loc, L, eps), D, self.free_bits)
    extra = self.reg_coef * t_mmd(z, prior) if self.reg_coef is not None else 0.0
    loss = -llk.mean() + self.beta * kl.mean() + extra
    return dict(loss=loss, llk=llk, kl=kl, extra=extra, p=p, z=z, h_e=h_e)

  def loss_and_grads(self, P, x, eps, prior=None):
    """P: {key: array}; -> (values as numpy, {key: gradient}, d loss / d p)"""
    T = {k: torch.tensor(np.asarray(v), dtype=torch.float64, requires_grad=True) for k, v in P.items()}
    t = lambda a: None if a is None else torch.tensor(np.asarray(a), dtype=torch.float64)
    out = self.forward(T, t(x), t(eps), t(prior))
    out['p'].retain_grad()
    out['loss'].backward()
    G = {k: v.grad.numpy() for k, v in T.items()}
    dp = out['p'].grad.numpy()
    return {k: (v.detach().numpy() if torch.is_tensor(v) else v) for k, v in out.items()}, G, dp
