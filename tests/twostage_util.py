"""TwoStageVAE's second stage restated in float64 with torch autograd (two_stage_vae.py:68-97, 181-192;
layers/latents.py:23-45), and the scaffolding the tests of tests/test_two_stage.py share.

  encoder2      z [B, D] -> Dense(units_i, act) ... -> Concatenate([z, h])
  latents2      Dense(D + H -> 2 Du): loc = p[:, :Du], scale = softplus(p[:, Du:]), prior N(0, I)
  decoder2      u [B, Du] -> Dense(units[::-1]_i, act) ... -> Concatenate([u, g])
  observation2  Dense(Du + H' -> 2 D), used as a likelihood: log p(z | u)
  loss          -mean(llk - kl), beta not applied

Parameters travel as {checkpoint name: tensor} with the names of Stage2Network.names()."""
import math

import numpy as np
import torch

F64 = torch.float64
LOG2PI = math.log(2.0 * math.pi)


def softplus(x):
  return torch.clamp(x, min=0) + torch.log1p(torch.exp(-x.abs()))


def act(name, v):
  if name == 'relu':
    return torch.clamp(v, min=0)
  if name == 'elu':
    return torch.where(v > 0, v, torch.expm1(torch.clamp(v, max=0)))
  assert name in ('linear', None), name
  return v


def act_grad_from_output(name, y):
  """the derivative of the activation expressed from its output, as the kernels take it"""
  if name == 'relu':
    return (y > 0).to(y.dtype)
  if name == 'elu':
    return torch.where(y > 0, torch.ones_like(y), y + 1)
  return torch.ones_like(y)


def log_prob(loc, scale, t):
  """Independent(Normal(loc, scale), 1).log_prob(t)"""
  return (-0.5 * ((t - loc) / scale) ** 2 - torch.log(scale) - 0.5 * LOG2PI).sum(-1)


def kl(loc, scale, z, form):
  """KL of q = N(loc, scale) against N(0, I): 'mc' log q(z) - log p(z) at the sample z, 'analytic' KL(q || p),
  'forward' KL(p || q) (reverse=False)"""
  if form == 'mc':
    return log_prob(loc, scale, z) - log_prob(torch.zeros_like(loc), torch.ones_like(scale), z)
  if form == 'analytic':
    return 0.5 * (scale ** 2 + loc ** 2 - 1.0 - 2.0 * torch.log(scale)).sum(-1)
  assert form == 'forward', form
  return (torch.log(scale) + 0.5 * (1.0 + loc ** 2) / scale ** 2 - 0.5).sum(-1)


FORMS = {'mc': 0, 'analytic': 1, 'forward': 2}   # odin_latent_fwd's `analytic`


def skip_head(x, h, W, b):
  """Dense over Concatenate([x, h]): the input comes first"""
  return torch.cat([x, h], -1) @ W + b


def stack(x, P, net, n, activation):
  h = x
  for i in range(n):
    h = act(activation, h @ P[f'{net}/{net.capitalize()}_{i}/kernel'] + P[f'{net}/{net.capitalize()}_{i}/bias'])
  return h


def posterior2(P, z, n, activation):
  """-> (loc, scale) of q(u | z)"""
  p = skip_head(z, stack(z, P, 'encoder2', n, activation), P['latents2/kernel'], P['latents2/bias'])
  Du = p.shape[-1] // 2
  return p[:, :Du], softplus(p[:, Du:])


def likelihood2(P, u, n, activation):
  """-> (loc, scale) of p(z | u)"""
  p = skip_head(u, stack(u, P, 'decoder2', n, activation), P['observation2/kernel'], P['observation2/bias'])
  D = p.shape[-1] // 2
  return p[:, :D], softplus(p[:, D:])


def stage2_elbo(P, z, eps2, n, activation, form='mc', free_bits=None):
  """-> (loss, llk [B], kl [B]) with z the first stage's cached sample (data: no gradient)"""
  loc, scale = posterior2(P, z, n, activation)
  u = loc + scale * eps2
  k = kl(loc, scale, u, form)
  if free_bits is not None:
    k = torch.clamp(k, min=free_bits * loc.shape[-1])
  ll = log_prob(*likelihood2(P, u, n, activation), z)
  return -(ll - k).mean(), ll, k


def params64(net, grad=True):
  """the network's parameters as float64 leaves, by checkpoint name"""
  P = {}
  for name, off, shp in net.names():
    t = net.params[off:off + int(np.prod(shp))].view(shp).detach().cpu().to(F64).clone()
    P[name] = t.requires_grad_(True) if grad else t
  return P


def flat_views(net, flat):
  return {name: flat[off:off + int(np.prod(shp))].view(shp).detach().cpu().numpy().astype(np.float64)
          for name, off, shp in net.names()}


def close(got, ref, tol=1e-4):
  got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
  scale = max(float(np.abs(ref).max()), 1e-30)
  err = float(np.abs(got - ref).max())
  assert err <= tol * scale, (err, scale)


def gap_threshold(values, bound):
  """a threshold in the middle of the widest gap between two of `values` (free bits that clamp some samples and not
  others) among the gaps with a positive middle -- a single-sample KL may be negative, a negative free_bits switches the
  clamp off; asserts that no value sits within twice `bound` of it"""
  v = np.sort(np.asarray(values, np.float64))
  assert len(v) >= 2
  mid, gap = 0.5 * (v[1:] + v[:-1]), np.diff(v)
  assert (mid > 0).any()
  thr = float(mid[int(np.argmax(np.where(mid > 0, gap, -1.0)))])
  assert np.abs(v - thr).min() > 2 * bound * max(1.0, np.abs(v).max()), (v, thr)
  assert (v < thr).any() and (v > thr).any()
  return float(thr)


def adam_ref(P, G, M, V, t, lr, b1=0.9, b2=0.999, e=1e-7):
  a = lr * np.sqrt(1 - b2 ** t) / (1 - b1 ** t)
  for k in P:
    M[k] = b1 * M[k] + (1 - b1) * G[k]
    V[k] = b2 * V[k] + (1 - b2) * G[k] ** 2
    P[k] = P[k] - a * M[k] / (np.sqrt(V[k]) + e)


def head_case(B, Dx, E, H, h_act, seed):
  """float32 operands of one head call: x, h (an output of `h_act`: zeros under relu, values above -1 under elu), the
  Dense kernel and bias, a target and an upstream gradient"""
  rng = np.random.default_rng(seed)
  N = 2 * E
  x = rng.standard_normal((B, Dx))
  h = act(h_act, torch.tensor(rng.standard_normal((B, H)))).numpy()
  W = rng.standard_normal((Dx + H, N)) * (1.0 / math.sqrt(Dx + H))
  b = rng.standard_normal(N) * 0.3
  t = rng.standard_normal((B, E))
  dp = rng.standard_normal((B, N)) * 0.5
  return tuple(a.astype(np.float32) for a in (x, h, W, b, t, dp))
