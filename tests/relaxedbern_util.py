"""float64 restatement of the relaxed Bernoulli (binary Concrete) posterior 'relaxedbernoulli' (tests only).

Source of truth: RelaxedBernoulliLayer (odin/bay/layers/discrete.py:346 ff.), the default prior of a binary variable
(odin/bay/random_variable.py:149-154: Independent(Bernoulli(logits = 0))), the single-sample KL of
odin/bay/helpers.py:261-282 and TFP's documented RelaxedBernoulli = Sigmoid(Logistic(logits / tau, 1 / tau)).  TFP is not
available here: parity with the reference is unpinned, like the rest of the VAE oracle; the density is checked against
torch.distributions.LogitRelaxedBernoulli / RelaxedBernoulli instead (tests/test_latent_relaxedbern.py).

  n ~ Logistic(0, 1);  u = (l + n) / tau;  z = sigmoid(u)
  log q(z) = sum_d [ log tau - n_d - 2 softplus(-n_d) + softplus(u_d) + softplus(-u_d) ]          (log_q, n = tau u - l)
  log p(z) = -D log 2

Everything is torch float64 so that autograd can check the hand-written gradients; the hand gradients below are derived
from the formulas of this file -- not from the kernel.
"""
import math

import numpy as np
import torch

F64 = torch.float64
LOG2 = math.log(2.0)


def t64(a):
  return a.to(F64) if torch.is_tensor(a) else torch.as_tensor(np.asarray(a), dtype=F64)


def softplus(x):
  return torch.logaddexp(x, torch.zeros_like(x))


def logistic_of(U):
  """Logistic(0, 1) noise of a uniform draw"""
  return torch.log(U) - torch.log1p(-U)


def relax(l, n, tau):
  """-> (u, z = sigmoid(u))"""
  u = (l + n) / tau
  return u, torch.sigmoid(u)


def log_q_logit(l, u, tau):
  """Logistic(l / tau, 1 / tau).log_prob(u): the density of u itself; its standardised argument tau u - l is the noise"""
  n = tau * u - l
  return (math.log(tau) - n - 2.0 * softplus(-n)).sum(-1)


def log_jacobian(u):
  """-log |dz/du| summed over the units: z = sigmoid(u), dz/du = z (1 - z) = exp(-softplus(u) - softplus(-u))"""
  return (softplus(u) + softplus(-u)).sum(-1)


def log_q(l, u, tau):
  """log q(z) at z = sigmoid(u): the logit-space density pushed through Sigmoid"""
  return log_q_logit(l, u, tau) + log_jacobian(u)


def log_p(z):
  """Independent(Bernoulli(logits = 0)).log_prob on [0, 1]^D: the constant -D log 2"""
  return torch.full(z.shape[:-1], -z.shape[-1] * LOG2, dtype=F64)


def kl_mc(l, n, tau):
  u, z = relax(l, n, tau)
  return log_q(l, u, tau) - log_p(z)


def kl_bernoulli(l):
  """Jang et al.: KL(Bernoulli(sigmoid(l)) || Bernoulli(1/2)) summed over the units; pi log pi = -pi softplus(-l)"""
  pi = torch.sigmoid(l)
  return (-pi * softplus(-l) - (1.0 - pi) * softplus(l) + LOG2).sum(-1)


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


def latent_fwd(p, n, tau, analytic, free_bits=None, capacity=None):
  """-> z, kl (after the clamps), fbmask, kl before the clamps"""
  l, n = t64(p), t64(n)
  raw = kl_bernoulli(l) if analytic else kl_mc(l, n, tau)
  kl, m = clamp(raw, l.shape[-1], free_bits, capacity)
  return relax(l, n, tau)[1], kl, m, raw


def latent_bwd(p, n, G, fbmask, klw, tau, analytic):
  """dl [B, D] of  sum_b (klw fbmask_b kl_b + G_b . z_b)  by hand.
  z = sigmoid(u), u = (l + n) / tau: dz/dl = z (1 - z) / tau.  Monte Carlo: the noise terms of log q do not depend on l,
  d/du [softplus(u) + softplus(-u)] = sigmoid(u) - sigmoid(-u) = 2 z - 1, and log p is constant.  Closed form: with
  H(pi) = pi log pi + (1 - pi) log(1 - pi), dH/dpi = logit(pi) = l and dpi/dl = pi (1 - pi)."""
  l, n, G, fbmask = t64(p), t64(n), t64(G), t64(fbmask)
  _, z = relax(l, n, tau)
  w = (klw * fbmask)[:, None]
  dl = G * z * (1.0 - z) / tau
  if analytic:
    pi = torch.sigmoid(l)
    return dl + w * pi * (1.0 - pi) * l
  return dl + w * (2.0 * z - 1.0) / tau


class RelaxedBernRef:
  """The whole step in torch float64 autograd over oracle.torch_ref's layers: encoder -> Dense(D) -> relaxed Bernoulli
  posterior -> decoder -> Bernoulli log-likelihood; loss = -mean llk + beta mean kl."""

  def __init__(self, enc, dec, D, tau=0.5, analytic=False, beta=1.0, free_bits=None):
    self.enc, self.dec, self.D, self.tau = list(enc), list(dec), int(D), float(tau)
    self.analytic, self.beta, self.free_bits = bool(analytic), float(beta), free_bits

  def forward(self, T, x, n):
    from oracle.torch_ref import TorchVAE, t_seq
    B = x.shape[0]
    h_e = t_seq(self.enc, TorchVAE._sub(T, 'enc'), x)
    p = h_e @ T[('lat', 'w')] + T[('lat', 'b')]
    u, z = relax(p, n, self.tau)
    h_d = t_seq(self.dec, TorchVAE._sub(T, 'dec'), z)
    llk = (x * h_d - softplus(h_d)).reshape(B, -1).sum(1)
    raw = kl_bernoulli(p) if self.analytic else log_q(p, u, self.tau) - log_p(z)
    kl, _ = clamp(raw, self.D, self.free_bits)
    loss = -llk.mean() + self.beta * kl.mean()
    return dict(loss=loss, llk=llk, kl=kl, p=p, z=z, h_e=h_e)

  def loss_and_grads(self, P, x, n):
    """P: {key: array}; -> (values as numpy, {key: gradient}, d loss / d p)"""
    T = {k: torch.tensor(np.asarray(v), dtype=F64, requires_grad=True) for k, v in P.items()}
    out = self.forward(T, t64(x), t64(n))
    out['p'].retain_grad()
    out['loss'].backward()
    G = {k: v.grad.numpy() for k, v in T.items()}
    dp = out['p'].grad.numpy()
    return {k: (v.detach().numpy() if torch.is_tensor(v) else v) for k, v in out.items()}, G, dp
