"""float64 restatement of the relaxed one-hot (Concrete / Gumbel-softmax) posterior 'relaxedonehot' (tests only).

Source of truth: RelaxedOneHotCategoricalLayer (odin/bay/layers/discrete.py:286-343), the default prior of a one-hot
variable (odin/bay/random_variable.py:141-146: OneHotCategorical with equal logits), the single-sample KL of
odin/bay/helpers.py:261-282 and TFP's documented RelaxedOneHotCategorical = Exp(ExpRelaxedOneHotCategorical).  TFP is not
available here: parity with the reference is unpinned, like the rest of the VAE oracle; the density is checked against
torch.distributions.RelaxedOneHotCategorical instead (tests/test_latent_concrete.py).

  u = (l + g) / tau;  y = u - logsumexp(u);  z = exp(y)
  log q(z) = lgamma(K) + (K - 1) log tau + sum_k log_softmax(l - tau y)_k - sum_k y_k          (log_q)
           = lgamma(K) + (K - 1) log tau - sum_k g_k - K logsumexp(-g) - sum_k y_k              (log_q_noise)
  log p(z) = -log K sum_k z_k

Everything is torch float64 so that autograd can check the hand-written gradients; the hand gradients below are derived
from the formulas of this file -- not from the kernel.
"""
import math

import numpy as np
import torch

F64 = torch.float64


def t64(a):
  return a.to(F64) if torch.is_tensor(a) else torch.as_tensor(np.asarray(a), dtype=F64)


def softplus(x):
  return torch.logaddexp(x, torch.zeros_like(x))


def relax(l, g, tau):
  """-> (y = log z, z)"""
  y = torch.log_softmax((l + g) / tau, -1)
  return y, torch.exp(y)


def log_const(K, tau):
  return math.lgamma(K) + (K - 1) * math.log(tau)


def log_q(l, y, tau):
  """ExpRelaxedOneHotCategorical.log_prob(y) pushed through Exp (the -sum y of the change of variables)"""
  K = l.shape[-1]
  return log_const(K, tau) + torch.log_softmax(l - tau * y, -1).sum(-1) - y.sum(-1)


def log_q_noise(g, y, tau):
  """the same number from the noise: l - tau y = -g + tau logsumexp(u), and log_softmax drops the shift"""
  K = g.shape[-1]
  return log_const(K, tau) - g.sum(-1) - K * torch.logsumexp(-g, -1) - y.sum(-1)


def log_p(z):
  return -math.log(z.shape[-1]) * z.sum(-1)


def kl_mc(l, g, tau):
  y, z = relax(l, g, tau)
  return log_q(l, y, tau) - log_p(z)


def kl_categorical(l):
  """Jang et al.: KL(Categorical(softmax(l)) || uniform)"""
  lp = torch.log_softmax(l, -1)
  return (lp.exp() * (lp + math.log(l.shape[-1]))).sum(-1)


def clamp(kl, K, free_bits=None, capacity=None):
  """-> (kl after free bits / capacity, fbmask): max(kl, free_bits K), then |kl - C| with the sign in the mask"""
  m = torch.ones_like(kl)
  if free_bits is not None:
    thr = free_bits * K
    hit = ~(kl > thr)
    m = torch.where(hit, torch.zeros_like(m), m)
    kl = torch.where(hit, torch.full_like(kl, thr), kl)
  if capacity is not None:
    d = kl - capacity
    m = m * torch.sign(d)
    kl = d.abs()
  return kl, m


def latent_fwd(p, g, tau, analytic, free_bits=None, capacity=None):
  """-> z, kl (after the clamps), fbmask, kl before the clamps"""
  l, g = t64(p), t64(g)
  raw = kl_categorical(l) if analytic else kl_mc(l, g, tau)
  kl, m = clamp(raw, l.shape[-1], free_bits, capacity)
  return relax(l, g, tau)[1], kl, m, raw


def latent_bwd(p, g, G, fbmask, klw, tau, analytic):
  """dl [B, K] of  sum_b (klw fbmask_b kl_b + G_b . z_b)  by hand.
  z = softmax(u), u = (l + g) / tau: dz_k/dl_j = z_k (delta_kj - z_j) / tau, so G . z gives z_j (G_j - G . z) / tau.
  Monte Carlo: log q = const(g) - sum_k y_k with dy_k/du_j = delta_kj - z_j, so dlog q/dl_j = -(1 - K z_j) / tau; log p is
  -log K on the whole simplex, its gradient vanishes.  Closed form: d/dl_j sum_k pi_k (log pi_k + log K) =
  pi_j (log pi_j - sum_k pi_k log pi_k)."""
  l, g, G, fbmask = t64(p), t64(g), t64(G), t64(fbmask)
  K = l.shape[-1]
  _, z = relax(l, g, tau)
  w = (klw * fbmask)[:, None]
  dl = z * (G - (G * z).sum(-1, keepdim=True)) / tau
  if analytic:
    lp = torch.log_softmax(l, -1)
    pi = lp.exp()
    return dl + w * pi * (lp - (pi * lp).sum(-1, keepdim=True))
  return dl - w * (1.0 - K * z) / tau


class ConcreteRef:
  """The whole step in torch float64 autograd over oracle.torch_ref's layers: encoder -> Dense(K) -> relaxed one-hot
  posterior -> decoder -> Bernoulli log-likelihood; loss = -mean llk + beta mean kl."""

  def __init__(self, enc, dec, K, tau=0.5, analytic=False, beta=1.0, free_bits=None):
    self.enc, self.dec, self.K, self.tau = list(enc), list(dec), int(K), float(tau)
    self.analytic, self.beta, self.free_bits = bool(analytic), float(beta), free_bits

  def forward(self, T, x, g):
    from oracle.torch_ref import TorchVAE, t_seq
    B = x.shape[0]
    h_e = t_seq(self.enc, TorchVAE._sub(T, 'enc'), x)
    p = h_e @ T[('lat', 'w')] + T[('lat', 'b')]
    y, z = relax(p, g, self.tau)
    h_d = t_seq(self.dec, TorchVAE._sub(T, 'dec'), z)
    llk = (x * h_d - softplus(h_d)).reshape(B, -1).sum(1)
    raw = kl_categorical(p) if self.analytic else log_q(p, y, self.tau) - log_p(z)
    kl, _ = clamp(raw, self.K, self.free_bits)
    loss = -llk.mean() + self.beta * kl.mean()
    return dict(loss=loss, llk=llk, kl=kl, p=p, z=z, h_e=h_e)

  def loss_and_grads(self, P, x, g):
    """P: {key: array}; -> (values as numpy, {key: gradient}, d loss / d p)"""
    T = {k: torch.tensor(np.asarray(v), dtype=F64, requires_grad=True) for k, v in P.items()}
    out = self.forward(T, t64(x), t64(g))
    out['p'].retain_grad()
    out['loss'].backward()
    G = {k: v.grad.numpy() for k, v in T.items()}
    dp = out['p'].grad.numpy()
    return {k: (v.detach().numpy() if torch.is_tensor(v) else v) for k, v in out.items()}, G, dp
