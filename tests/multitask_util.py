"""Float64 restatement of MultitaskVAE / SkiptaskVAE's label head and labelled step (multitask_vae.py:164-207,
variational_autoencoder.py:606-632) for tests/test_multitask.py -- plain torch formulas, differentiated by autograd, sharing
no code with the kernels of label_head.hip.

  z' = loc + softplus(raw) eps_y;  logits = z' W + b;  log p(y|z') = sum_k y_k log_softmax(logits)_k
  loss = -mean_u(llk_u - beta kl_u) - mean_s(llk_s - beta kl_s) - alpha mean_s log p(y_s | z')
(the two half-batch means are ADDED), an unlabelled step is the plain -mean(llk - beta kl) with a zero gradient for W, b.
"""
import numpy as np
import torch

F64 = torch.float64


def t64(a):
  return torch.as_tensor(np.asarray(a), dtype=F64)


def softplus(x):
  return torch.clamp(x, min=0) + torch.log1p(torch.exp(-x.abs()))


def label_logits(loc, raw, eps_y, W, b):
  return (loc + softplus(raw) * eps_y) @ W + b


def label_log_prob(logits, y):
  """sum_k y_k (logit_k - logsumexp(logits)): OneHotCategorical._log_prob, soft labels included"""
  return (y * (logits - torch.logsumexp(logits, -1, keepdim=True))).sum(-1)


def close(got, ref, tol=1e-4):
  """within `tol` of the reference tensor's own maximum (tests/twostage_util.close), and finite"""
  got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
  scale = max(float(np.abs(ref).max()), 1e-30)
  err = float(np.abs(got - ref).max())
  assert np.isfinite(got).all() and err <= tol * scale, (err, scale)


def head_case(B, Bs, D, K, seed, soft=False):
  """float32 operands of one label-head call, as float32 values: p [B, 2 D], eps_y [Bs, D], W [D, K], b [K], y [Bs, K]"""
  rng = np.random.default_rng(seed)
  p = rng.standard_normal((B, 2 * D))
  eps = rng.standard_normal((Bs, D))
  W = rng.standard_normal((D, K)) / np.sqrt(D)
  b = 0.3 * rng.standard_normal(K)
  if soft:
    y = rng.random((Bs, K)) + 0.05
    y /= y.sum(-1, keepdims=True)
  else:
    y = np.eye(K)[rng.integers(0, K, Bs)]
  return tuple(a.astype(np.float32) for a in (p, eps, W, b, y))


def head_ref(p, eps, W, b, y, c, row0):
  """-> dict: logits, llk [Bs], value, dloc / dscale [B, D] (zero outside the labelled block), dW, db -- the gradients of
  c * sum_b llk_b, dscale with respect to the scale softplus(raw)"""
  p, eps, W, b, y = (t64(a) for a in (p, eps, W, b, y))
  Bs, D = eps.shape
  loc = p[row0:row0 + Bs, :D].clone().requires_grad_(True)
  scale = softplus(p[row0:row0 + Bs, D:]).clone().requires_grad_(True)
  W, b = W.clone().requires_grad_(True), b.clone().requires_grad_(True)
  logits = (loc + scale * eps) @ W + b
  llk = label_log_prob(logits, y)
  (c * llk.sum()).backward()
  dloc, dscale = torch.zeros(p.shape[0], D, dtype=F64), torch.zeros(p.shape[0], D, dtype=F64)
  dloc[row0:row0 + Bs], dscale[row0:row0 + Bs] = loc.grad, scale.grad
  return dict(logits=logits.detach().numpy(), llk=llk.detach().numpy(), value=float(llk.detach().mean()), dloc=dloc.numpy(),
              dscale=dscale.numpy(), dW=W.grad.numpy(), db=b.grad.numpy())


class StepRef:
  """one step of the model over given parameters {engine key: array}: float64 autograd through oracle.torch_ref.t_seq.
  observation: 'bernoulli' | 'nb'; kl_form: 'mc' | 'analytic'; free_bits: None | nats per latent unit."""

  def __init__(self, enc, dec, zdim, observation, kl_form='mc', free_bits=None):
    self.enc, self.dec, self.D = list(enc), list(dec), int(zdim)
    self.observation, self.kl_form, self.free_bits = observation, kl_form, free_bits

  def _elbo_parts(self, T, x, eps):
    from oracle.torch_ref import TorchVAE, t_seq
    from tests import nb_util as nb
    D = self.D
    h0 = nb.lognorm(x) if self.enc[0][0] == 'lognorm' else x
    h_e = t_seq(self.enc, TorchVAE._sub(T, 'enc'), h0)
    p = h_e @ T[('lat', 'w')] + T[('lat', 'b')]
    loc, raw = p[:, :D], p[:, D:]
    scale = softplus(raw)
    z = loc + scale * eps
    h_d = t_seq(self.dec, TorchVAE._sub(T, 'dec'), z)
    if self.observation == 'bernoulli':
      llk = (x * h_d - softplus(h_d)).reshape(x.shape[0], -1).sum(1)
    else:
      llk = nb.log_prob_sum(h_d, x, self.observation == 'zinb')
    if self.kl_form == 'analytic':
      kl = 0.5 * (scale ** 2 + loc ** 2 - 1.0 - 2.0 * torch.log(scale)).sum(-1)
    else:
      kl = (0.5 * (z ** 2 - eps ** 2) - torch.log(scale)).sum(-1)
    if self.free_bits is not None:
      kl = torch.clamp(kl, min=self.free_bits * D)
    return llk, kl, loc, raw

  def loss_and_grads(self, P, x, eps, beta, y=None, eps_y=None, alpha=10.0):
    """x = cat(x_u, x_s) when y [B / 2, K] is given.  -> (dict of the loss and the five metrics, {key: gradient})"""
    T = {k: t64(v).clone().requires_grad_(True) for k, v in P.items()}
    x, eps = t64(x), t64(eps)
    llk, kl, loc, raw = self._elbo_parts(T, x, eps)
    if y is None:
      loss = -(llk - beta * kl).mean()
      f = {'loss': loss, 'uns/llk': llk.mean(), 'uns/kl': beta * kl.mean()}
    else:
      h = x.shape[0] // 2
      lly = label_log_prob(label_logits(loc[h:], raw[h:], t64(eps_y), T[('lab', 'w')], T[('lab', 'b')]), t64(y))
      loss = -(llk[:h] - beta * kl[:h]).mean() - (llk[h:] - beta * kl[h:]).mean() - alpha * lly.mean()
      f = {'loss': loss, 'uns/llk': llk[:h].mean(), 'uns/kl': beta * kl[:h].mean(), 'sup/llk': llk[h:].mean(),
           'sup/kl': beta * kl[h:].mean(), 'sup/llk_y': alpha * lly.mean()}
    loss.backward()
    G = {k: (v.grad.numpy() if v.grad is not None else np.zeros(tuple(v.shape))) for k, v in T.items()}
    return {k: float(v.detach()) for k, v in f.items()}, G


def adam_ref(P, G, M, V, t, lr, b1=0.9, b2=0.999, e=1e-7, clip=None):
  """Keras Adam over float64 dictionaries, in place; `clip`: global_clipnorm (clip_by_global_norm ahead of the update)"""
  if clip is not None:
    nrm = np.sqrt(sum(float((g ** 2).sum()) for g in G.values()))
    sc = clip / max(nrm, clip)
    G = {k: g * sc for k, g in G.items()}
  a = lr * np.sqrt(1 - b2 ** t) / (1 - b1 ** t)
  for k in P:
    M[k] = b1 * M[k] + (1 - b1) * G[k]
    V[k] = b2 * V[k] + (1 - b2) * G[k] ** 2
    P[k] = P[k] - a * M[k] / (np.sqrt(V[k]) + e)
