"""Range-word audit of a live VAEEngine (tests only).

Every tensor that feeds a two-plane kernel travels with a range word: the fp32 bit pattern of max |t| (DESIGN 3.8,
odin_device.h: odin_range_shift / odin_act_needs_scale).  The kernels are exact relative to that word, so a step is
right only if the engine hands each consumer the word of the right tensor, the word is tight, and it was cleared
since the step before.  A word that is merely too large costs bits without any error, which no parity test at 1e-4
sees; this audit does.

    audit = RangeAudit(eng)          # installs itself as eng.debug_check_ranges (called in backward(), before the
    eng.forward(x, eps); eng.backward()   # slab reduction clears the words)
    audit.check_cleared()            # after a complete step, eager or graph-replayed

Checks, per audited step:
  (a) every word bounds its tensor: bound >= max|t|
  (b) every word is tight: bound <= TIGHT * max|t|, unless LOOSE names it (with its reason)
  (c) a plane consumer handed no word reads a tensor whose max lies in [2^-8, 2^15) (its unscaled body's window)
  (d) check_cleared(): after the step the engine's whole range_words buffer is zero
and it records what VAEEngine._jobs_cover returned (`cover`).
"""
from typing import Dict, List, Optional, Tuple

import numpy as np
import torch

from odin_ai_amd.engine import RANGE_WORDS

TIGHT = 1.0001           # the bar of tests/test_ops.py::test_data_gradient_range_contract
ACT_WINDOW = (2.0 ** -8, 2.0 ** 15)   # odin_act_needs_scale: activations inside it take the unscaled body

# words that are looser than max|t| by design: name -> reason.  Only (a) applies to them.
LOOSE: Dict[str, str] = {
    # FactorVAE: the forward-only engine of the second half batch folds its maxima into the owner's activation words
    # (VAEEngine(range_words=...)): the words bound both half batches, the owner's tensors hold one of them
    'shared_act': 'words shared with a forward-only engine (max over both half batches)',
}


def _block_max(words: torch.Tensor, addr: int) -> float:
  i = (addr - words.data_ptr()) // 4
  assert 0 <= i and i + RANGE_WORDS <= words.numel(), 'word outside the engine buffer'
  return float(words[i:i + RANGE_WORDS].view(torch.float32).max().item())


def _tmax(t: torch.Tensor) -> float:
  return float(torch.nan_to_num(t, nan=0.0, posinf=0.0, neginf=0.0).abs().max().item())


class RangeAudit:

  def __init__(self, eng, shared_acts: bool = False, fail_fast: bool = True):
    self.eng, self.shared_acts, self.fail_fast = eng, bool(shared_acts), fail_fast
    self.steps: List[List[Tuple[str, str, float, float]]] = []   # per audited step: (name, kind, bound, max)
    self.failures: List[str] = []
    self.cover: List[bool] = []
    eng.debug_check_ranges = self
    orig = eng._jobs_cover

    def recording(jobs):
      r = orig(jobs)
      self.cover.append(bool(r))
      return r
    eng._jobs_cover = recording

  # -- the words of one step --------------------------------------------------------------
  def _entries(self, eng):
    """(name, kind, word address or None, tensor) for every word a consumer of this step reads; kind: 'strict',
    'loose:<key>' or 'none' (a plane consumer that reads no word)"""
    enc, dec = eng.enc, eng.dec
    ne, nd = len(eng.enc_recs), len(eng.dec_recs)
    out = []
    neck_b = eng._bwd_neck()
    tail = eng._used_fused or eng._used_head
    # gradient words (gouts[i]: dL / d pre-activation of layer i)
    dec_lo = 1 if neck_b else 0            # (gouts[0] stays inside the neck's backward launch)
    dec_hi = nd - 1 if tail else nd        # (the fused tail / head writes gouts[nd - 2] directly)
    for prog, name, lo, hi in ((enc, 'enc', 0, ne), (dec, 'dec', dec_lo, dec_hi)):
      for i in range(lo, hi):
        w = prog.dy_word[i]
        if w is None:
          continue
        kind = 'strict' if w == prog.word(i) else 'foreign'
        out.append((f'{name}.gouts[{i}] ({prog.recs[i].kind})', kind, w, prog.gouts[i]))
    # activation words (outs[i - 1], read by layer i's plane kernels)
    act = 'loose:shared_act' if self.shared_acts else 'strict'
    dec_start = 2 if eng._used_neck else (1 if eng._used_block else 0)
    for prog, name, lo, hi in ((enc, 'enc', 1, ne), (dec, 'dec', max(1, dec_start), nd - 1 if tail else nd)):
      for i in range(lo, hi):
        if eng._used_neck and prog is enc and i >= ne - 2:
          continue   # (conv3 and the projection run inside the neck launch: its input word is checked below)
        w = prog.x_word[i]
        if w is not None:
          out.append((f'{name}.outs[{i - 1}] -> layer {i}', act if w == prog.aword(i - 1) else 'foreign', w,
                      prog.outs[i - 1]))
        elif prog.reads_x[i]:
          out.append((f'{name}.outs[{i - 1}] -> layer {i} (no word)', 'none', None, prog.outs[i - 1]))
    if enc.reads_x[0]:
      out.append(('enc input -> layer 0 (no word)', 'none', None, eng.x))
    if eng._used_neck:
      w = enc.y_word[ne - 3]
      out.append((f'enc.outs[{ne - 3}] -> neck (x_amax)', act if w == enc.aword(ne - 3) else 'foreign', w,
                  enc.outs[ne - 3]))
    return out

  def __call__(self, eng) -> None:
    if eng.device.type == 'cuda':
      torch.cuda.synchronize(eng.device)
    words = eng.range_words
    rec, bad = [], []
    for name, kind, w, t in self._entries(eng):
      m = _tmax(t)
      if kind == 'none':
        rec.append((name, kind, float('nan'), m))
        if m != 0.0 and not (ACT_WINDOW[0] <= m < ACT_WINDOW[1]):
          bad.append(f'(c) {name}: no word and max|t| = {m:.6g} outside [2^-8, 2^15)')
        continue
      if kind == 'foreign':
        bad.append(f'{name}: handed a word that is not its own')
        continue
      b = _block_max(words, w)
      rec.append((name, kind, b, m))
      if not b >= m:
        bad.append(f'(a) {name}: word {b:.6g} < max|t| = {m:.6g}')
      elif kind == 'strict' and b > TIGHT * m:
        bad.append(f'(b) {name}: word {b:.6g} > {TIGHT} * max|t| = {m:.6g} (x{b / max(m, 1e-45):.4g})')
    self.steps.append(rec)
    if bad:
      self.failures += [f'step {len(self.steps)}: {s}' for s in bad]
      if self.fail_fast:
        raise AssertionError('range-word audit failed:\n  ' + '\n  '.join(bad))

  # -- after a complete step ------------------------------------------------------------
  def check_cleared(self) -> None:
    """(d) the engine's whole range_words buffer is zero after a complete step"""
    eng = self.eng
    if eng.device.type == 'cuda':
      torch.cuda.synchronize(eng.device)
    nz = int((eng.range_words != 0).sum().item())
    assert nz == 0, f'(d) {nz} range-word entries not cleared after the step'

  def check_cover(self, expect: Optional[bool] = None) -> None:
    """_jobs_cover: True for every engine without direct-write layers (a missing or doubled gradient slice would
    otherwise fall back silently to the separate norm launch)"""
    eng = self.eng
    if expect is None:
      expect = not (any(eng.enc.wdirect) or any(eng.dec.wdirect))
    if expect:
      assert all(self.cover), f'_jobs_cover returned {self.cover}'

  def n_checked(self) -> int:
    return sum(len(s) for s in self.steps)


def bern_targets(shape, seed=3):
  """Bernoulli targets outside [0, 1], every fifth exactly 0 and every fifth exactly 1"""
  x = np.random.default_rng(seed).uniform(-2.0, 6.0, size=shape)
  x.reshape(-1)[::5] = 0.0
  x.reshape(-1)[1::5] = 1.0
  return x
