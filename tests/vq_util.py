"""float64 restatement of the vector quantiser of VQVAE (tests only).

Source of truth: odin/bay/distributions/vector_quantizer.py and odin/bay/vi/autoencoder/vq_vae.py of the reference,
restated in numpy / torch float64.  The reference's `_elbo` override is never called by its base class; the evident
intent is restated here: loss = -mean llk + beta * L * log K + commitment (+ latents), then the moving-average update.
"""
import math

import numpy as np
import torch


def distances64(codes, codebook, chunk=256):
  """[N, K] float64 squared distances sum_d (c - e)^2 (never the expanded form)"""
  c = np.asarray(codes, np.float64)
  e = np.asarray(codebook, np.float64)
  out = np.empty((c.shape[0], e.shape[0]), np.float64)
  for i in range(0, c.shape[0], chunk):
    d = c[i:i + chunk, None, :] - e[None, :, :]
    out[i:i + chunk] = (d * d).sum(-1)
  return out


def assign64(codes, codebook):
  """-> idx [N] (ties: the smallest index, as np.argmin), z_q, m, cnt, dist [N, K]"""
  dist = distances64(codes, codebook)
  idx = dist.argmin(1)
  e = np.asarray(codebook, np.float64)
  zq = e[idx]
  m = float(((np.asarray(codes, np.float64) - zq) ** 2).mean())
  cnt = np.bincount(idx, minlength=e.shape[0])
  return idx, zq, m, cnt, dist


def near_ties(dist, rel=1e-5):
  """rows whose relative gap between the best and the second-best distance is below `rel`"""
  if dist.shape[1] < 2:
    return np.zeros(dist.shape[0], bool)
  p = np.partition(dist, 1, axis=1)
  best, second = p[:, 0], p[:, 1]
  return (second - best) < rel * np.maximum(second, 1e-300)


def check_assignment(idx_k, dist, rel=1e-5, cap=0.01):
  """The issue's rule: a near-tie row may pick any code whose distance is within `rel` of the minimum; every other
  row must give the exact index; near ties are at most `cap` of the rows."""
  idx_k = np.asarray(idx_k).astype(np.int64)
  ref = dist.argmin(1)
  nt = near_ties(dist, rel)
  assert nt.mean() <= cap, f'{nt.sum()} near-tie rows of {len(nt)}'
  assert ((idx_k >= 0) & (idx_k < dist.shape[1])).all()
  bad = (idx_k != ref) & ~nt
  assert not bad.any(), f'{bad.sum()} rows with a wrong index, first {np.nonzero(bad)[0][:5]}'
  rows = np.nonzero(nt)[0]
  dmin = dist[rows].min(1)
  got = dist[rows, idx_k[rows]]
  assert (got <= dmin * (1 + rel)).all(), 'a near-tie row chose a code beyond 1e-5 of the minimum'
  return int(nt.sum())


def bwd64(codes, codebook, idx, dzq, commitment):
  """dcodes (straight through + commitment) and dcodebook of the `latents` term, from GIVEN assignments"""
  c = np.asarray(codes, np.float64)
  e = np.asarray(codebook, np.float64)
  idx = np.asarray(idx).astype(np.int64)
  n = c.size
  zq = e[idx]
  dcodes = np.asarray(dzq, np.float64) + 2.0 * commitment / n * (c - zq)
  dcb = np.zeros_like(e)
  np.add.at(dcb, idx, 2.0 / n * (zq - c))
  return dcodes, dcb


def ema64(codes, idx, ema_counts, ema_means, decay, epsilon):
  c = np.asarray(codes, np.float64)
  idx = np.asarray(idx).astype(np.int64)
  K = len(ema_counts)
  cnt = np.bincount(idx, minlength=K).astype(np.float64)
  s = np.zeros((K, c.shape[1]), np.float64)
  np.add.at(s, idx, c)
  nc = decay * np.asarray(ema_counts, np.float64) + (1.0 - decay) * cnt
  nm = decay * np.asarray(ema_means, np.float64) + (1.0 - decay) * s
  return nc, nm, nm / (nc + epsilon)[:, None]


class VQRef:
  """Whole step in torch float64 autograd over oracle.torch_ref's layers, the stop_gradient structure by hand:
     z_st = c + (z_q - c).detach();  commitment = w * mean((c - z_q.detach())^2);  latents = mean((c.detach() - z_q)^2)"""

  def __init__(self, enc, dec, observation, n_codes, code_size=None, commitment=0.25, ema=False, beta=1.0):
    self.enc, self.dec, self.observation = list(enc), list(dec), observation
    self.K, self.Cs, self.cw, self.ema, self.beta = int(n_codes), code_size, float(commitment), bool(ema), float(beta)

  def forward(self, T, codebook, x, idx=None):
    """T: {key: float64 tensor} of the networks, codebook: float64 tensor [K, Cs], x: float64 tensor.  `idx`: impose
    the assignments (the kernel's, once check_assignment has accepted them) so that a near tie cannot split the
    comparison; None: the float64 argmin."""
    from oracle.torch_ref import LOG2PI, SOFTPLUS_INV_1, TorchVAE, t_seq
    import torch.nn.functional as F
    h = t_seq(self.enc, TorchVAE._sub(T, 'enc'), x)
    B, H = h.shape
    Cs = self.Cs or H
    L = H // Cs
    c = h.reshape(B * L, Cs)
    if idx is None:
      d = ((c.detach()[:, None, :] - codebook.detach()[None, :, :]) ** 2).sum(-1)
      idx = d.argmin(1)
    else:
      idx = torch.as_tensor(np.asarray(idx).astype(np.int64))
    zq = codebook[idx]
    m_c = ((c - zq.detach()) ** 2).mean()
    m_l = ((c.detach() - zq) ** 2).mean()
    z_st = c + (zq - c).detach()
    h_d = t_seq(self.dec, TorchVAE._sub(T, 'dec'), z_st.reshape(B, H))
    if self.observation == 'bernoulli':
      llk = (x * h_d - F.softplus(h_d)).reshape(B, -1).sum(1)
    else:
      C = x.shape[-1]
      oloc, raw = h_d[..., :C], h_d[..., C:]
      osc = F.softplus(raw + SOFTPLUS_INV_1) if self.observation == 'gaussian_softplus1' else raw
      llk = (-0.5 * ((x - oloc) / osc) ** 2 - torch.log(osc) - 0.5 * LOG2PI).reshape(B, -1).sum(1)
    kl = self.beta * L * math.log(self.K)
    extra = self.cw * m_c + (0.0 if self.ema else 1.0) * m_l
    loss = -llk.mean() + kl + extra
    return dict(loss=loss, llk=llk, kl=kl, extra=extra, m=m_c, idx=idx, codes=c, zq=zq, h_d=h_d)

  def loss_and_grads(self, P, codebook, x, idx=None):
    """P: {key: array} of the networks; -> (values as numpy, gradients {key: array} incl. ('vq', 'codebook') unless
    ema)"""
    T = {k: torch.tensor(np.asarray(v), dtype=torch.float64, requires_grad=True) for k, v in P.items()}
    cb = torch.tensor(np.asarray(codebook), dtype=torch.float64, requires_grad=not self.ema)
    out = self.forward(T, cb, torch.tensor(np.asarray(x), dtype=torch.float64), idx)
    out['loss'].backward()
    G = {k: (v.grad.numpy() if v.grad is not None else np.zeros(tuple(v.shape))) for k, v in T.items()}
    if not self.ema:
      G[('vq', 'codebook')] = cb.grad.numpy()
    return {k: (v.detach().numpy() if torch.is_tensor(v) else v) for k, v in out.items()}, G
