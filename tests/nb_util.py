"""Float64 restatement of the count observations ('nb' / 'zinb') and of LogNorm, the reference of
tests/test_count_observations.py.  For params = (a | l) or (a | l | pi) (planes, split on the last axis), r = e^a:

  llk     = lgamma(r + x) - lgamma(r) - lgamma(1 + x) - r softplus(l) - x softplus(-l)
  d/da    = r (psi(r + x) - psi(r) - softplus(l)),   d/dl = x sigmoid(-l) - r sigmoid(l),   mean = r e^l
  zinb:   t1 = llk - pi, t2 = softplus(-pi); log p = t1 - t2 where x > 1e-8, softplus(t1) - t2 otherwise; with s = sigmoid(t1)
          the NB gradients times 1 / s, d/dpi = -sigmoid(pi) / sigmoid(-pi) - s; mean = sigmoid(-pi) r e^l
  LogNorm: y = log1p(1e4 x / (sum_g x + 1e-8)) per row

Everything takes and returns float64 torch tensors, so autograd runs through it (the training-step reference).  In
float64 the two lgamma terms may be subtracted as they stand for the inputs of the tests: with a <= 9 (the random recipe)
lgamma(r) <= 7e4 and its rounding is 1e-11; the hand-placed (a, mu, x) = (20, 5, 3) has lgamma(r) = 9e9, rounding 1e-6
against a bound of 2e-4 (M = 120); the hand-placed a = 30 elements have x = 0, where `dlgamma` and `dpsi` return the exact
0.  torch's digamma likewise (r times its rounding: below 1e-11 for a <= 9).  The four term magnitudes M, Mg, Ml, Mz are
what the kernel's error is measured against."""
import numpy as np
import torch

F64 = torch.float64
sp = torch.nn.functional.softplus
ZERO_BELOW = 1e-8


def t64(a):
  return torch.as_tensor(np.asarray(a, dtype=np.float64), dtype=F64) if not torch.is_tensor(a) else a.to(F64)


def dlgamma(r, x):
  """lgamma(r + x) - lgamma(r), exactly 0 at x = 0"""
  return torch.where(x == 0, torch.zeros_like(x), torch.lgamma(r + x) - torch.lgamma(r))


def dpsi(r, x):
  """psi(r + x) - psi(r), exactly 0 at x = 0"""
  return torch.where(x == 0, torch.zeros_like(x), torch.digamma(r + x) - torch.digamma(r))


def nb_log_prob(a, l, x):
  """elementwise NegativeBinomial(total_count = e^a, logits = l).log_prob(x)"""
  r = torch.exp(a)
  return dlgamma(r, x) - torch.lgamma(1.0 + x) - r * sp(l) - x * sp(-l)


def nb_grads(a, l, x):
  """closed forms: (d llk / da, d llk / dl)"""
  r = torch.exp(a)
  return r * (dpsi(r, x) - sp(l)), x * torch.sigmoid(-l) - r * torch.sigmoid(l)


def zinb_log_prob(a, l, pi, x):
  t1, t2 = nb_log_prob(a, l, x) - pi, sp(-pi)
  return torch.where(x > ZERO_BELOW, t1 - t2, sp(t1) - t2)


def zinb_grads(a, l, pi, x):
  """closed forms: (d/da, d/dl, d/dpi)"""
  ga, gl = nb_grads(a, l, x)
  s = torch.sigmoid(nb_log_prob(a, l, x) - pi)
  pos = x > ZERO_BELOW
  w = torch.where(pos, torch.ones_like(s), s)
  return w * ga, w * gl, torch.where(pos, -torch.sigmoid(pi), torch.sigmoid(-pi) - s)


def magnitudes(a, l, x, pi=None):
  """-> dict(M, Mg, Ml[, Mz]): the sums of the term magnitudes the float32 errors are measured against"""
  r = torch.exp(a)
  M = dlgamma(r, x).abs() + torch.lgamma(1.0 + x) + r * sp(l) + x * sp(-l)
  out = dict(M=M, Mg=r * dpsi(r, x).abs() + r * sp(l), Ml=x * torch.sigmoid(-l) + r * torch.sigmoid(l))
  if pi is not None:
    out['Mz'] = M + 2.0 * sp(pi.abs())
  return out


def split(params, P):
  """params [..., P G] -> its P planes"""
  G = params.shape[-1] // P
  return tuple(params[..., p * G:(p + 1) * G] for p in range(P))


def log_prob(params, x, zi):
  """elementwise log p of params [..., P G] at x [..., G]"""
  return zinb_log_prob(*split(params, 3), x) if zi else nb_log_prob(*split(params, 2), x)


def log_prob_sum(params, x, zi):
  return log_prob(params, x, zi).reshape(x.shape[0], -1).sum(1)


def mean(params, zi):
  pl = split(params, 3 if zi else 2)
  m = torch.exp(pl[0] + pl[1])
  return torch.sigmoid(-pl[2]) * m if zi else m


def lognorm(x):
  return torch.log1p(1e4 * x / (x.sum(-1, keepdim=True) + 1e-8))


def draw(rng, shape, zi, a_lo=-6.0, a_hi=9.0):
  """the inputs of the kernel tests, as float32 values in float64 arrays: a uniform in [a_lo, a_hi], mu log-uniform in
  [1e-2, 3e3], l = log mu - a, x ~ NB(r, r / (r + mu)) with 30 % of the entries set to 0, pi = 3 N(0, 1)
  -> (params [..., P G], x [..., G])"""
  f32 = lambda v: np.asarray(v, np.float64).astype(np.float32).astype(np.float64)
  a = f32(rng.uniform(a_lo, a_hi, shape))
  mu = np.exp(rng.uniform(np.log(1e-2), np.log(3e3), shape))
  l = f32(np.log(mu) - a)
  r = np.exp(a)
  x = rng.negative_binomial(r, r / (r + mu)).astype(np.float64)
  x[rng.random(shape) < 0.3] = 0.0
  planes = [a, l] + ([f32(3.0 * rng.standard_normal(shape))] if zi else [])
  return np.concatenate(planes, -1), f32(x)


class CountRef:
  """The training step of a Gaussian-latent VAE with a count observation, float64 autograd through
  oracle.torch_ref.t_seq (which passes the ('lognorm',) tuple by: LogNorm is applied here): loss = -mean(llk - beta * kl)
  with the single-sample KL."""

  def __init__(self, enc, dec, zdim, beta, zi):
    self.enc, self.dec, self.D, self.beta, self.zi = list(enc), list(dec), int(zdim), float(beta), bool(zi)

  def loss_and_grads(self, P, x, eps):
    from oracle.torch_ref import TorchVAE, t_seq
    T = {k: torch.tensor(np.asarray(v), dtype=F64, requires_grad=True) for k, v in P.items()}
    xt, et = t64(x), t64(eps)
    D = self.D
    h0 = lognorm(xt) if self.enc[0][0] == 'lognorm' else xt
    h_e = t_seq(self.enc, TorchVAE._sub(T, 'enc'), h0)
    p = h_e @ T[('lat', 'w')] + T[('lat', 'b')]
    loc, scale = p[:, :D], sp(p[:, D:])
    z = loc + scale * et
    h_d = t_seq(self.dec, TorchVAE._sub(T, 'dec'), z)
    llk = log_prob_sum(h_d, xt, self.zi)
    kl = (0.5 * (z ** 2 - et ** 2) - torch.log(scale)).sum(-1)
    loss = -(llk - self.beta * kl).mean()
    loss.backward()
    G = {k: v.grad.detach().numpy() for k, v in T.items()}
    f = dict(h_d=h_d.detach().numpy(), llk=llk.detach().numpy(), kl=kl.detach().numpy(), loss=float(loss.detach()))
    return f, G
