"""Perturbation attributions on the device: occlusion sensitivity and RISE, ``_ModelBase.perturbation_attributions``.

The gradient methods of attribution.py all go through the same adjoints; these need none.  Hide a region of the input, run the
model's own forward, see how far the command moves: step m has an occlusion weight o_m(n, y, x) in [0, 1] per sample and pixel,
shared by the frames and channels of the occluded input, and

    saliency[n][pixel] = sum_m d_m[n] o_m / sum_m o_m        (+0 where no step hid the pixel)

is the mean change of the command over the steps that hid the pixel, weighted by how much they hid it.  The skeleton is
attribution.py's, its shared pieces in attr_pass.py: the occluded input is written into the model's own buffers (csrc/perturbation.hip: geeco_perturb_apply), the
model's forward runs untouched, the step's score (geeco_perturb_score) goes into the running sums (geeco_perturb_accumulate) and
one finish forms the map.  Nothing is copied to the host inside the loop and nothing is allocated there.
"""
from __future__ import annotations

import numpy as np
import torch

from . import ops
from .attr_pass import check_steps_seed, clean_inputs, periodic_operands
from .attribution import input_key
from .decoder import resolve_heads

METHODS = ('occlusion', 'rise')
SCORES = ('prediction', 'loss')
PASSES = {'rgb': ('rgb', 'depth'), 'target_rgb': ('target_rgb', 'target_depth')}      # a pass, by its first input: what it occludes


def _pair(v):
  return (v, v) if np.ndim(v) == 0 else tuple(v)


def check_perturbation_arguments(method, patch=None, stride=None, grid=7, keep_prob=0.5, steps=64, score='prediction', seed=0):
  """ValueError, with the reason, for arguments no model serves (``patch`` / ``stride`` None: the image decides, see the pass)."""
  if method not in METHODS:
    raise ValueError('perturbation_attributions: method=%r must be one of %s' % (method, ', '.join(repr(m) for m in METHODS)))
  if score not in SCORES:
    raise ValueError('perturbation_attributions: score=%r must be one of %s' % (score, ', '.join(repr(s) for s in SCORES)))
  if method == 'occlusion':
    for name, v in (('patch', patch), ('stride', stride)):
      if v is None:
        continue
      try:
        ok = len(_pair(v)) == 2 and all(int(e) == e and 1 <= int(e) < 1 << 30 for e in _pair(v))
      except (TypeError, ValueError):
        ok = False
      if not ok:
        raise ValueError('perturbation_attributions: %s=%r must be an integer >= 1 or a pair of them' % (name, v))
  else:
    if not isinstance(grid, (int, np.integer)) or not 2 <= int(grid) <= 31:
      raise ValueError('perturbation_attributions: grid=%r must be an integer in 2..31' % (grid,))
    if not 0.0 < float(keep_prob) < 1.0:
      raise ValueError('perturbation_attributions: keep_prob=%r must lie in (0, 1)' % (keep_prob,))
    check_steps_seed('perturbation_attributions', steps=steps)
  check_steps_seed('perturbation_attributions', seed=seed)


class Perturbations:
  """The perturbation pass of a model (mixed into ``graph._ModelBase``)."""

  _perturb = None      # the pass's buffers, allocated by the first call

  def check_perturbation_attributions(self):
    """ValueError, with the reason, unless ``perturbation_attributions`` serves this model (any ``training``)."""
    self._refuse_sparse_inputs('perturbation_attributions', 'an occluder on a slot would hide the frame in every window that holds it',
                               'the occluded input is written as float32 frames')

  def _perturb_buffers(self, passes, M):
    if self._perturb is None:
      f32 = dict(dtype=torch.float32, device=self.device)
      d = self.decoder
      self._perturb = dict(clean={}, fill={}, sums={}, scores={}, preds0=torch.empty_like(d.preds), w=torch.empty(d.OT, **f32),
                           losses=torch.empty(2, self.N, dtype=torch.float64, device=self.device))
    p = self._perturb
    for name in passes:
      for k in PASSES[name]:
        if k in self.inputs and k not in p['clean']:
          p['clean'][k] = torch.empty_like(self.inputs[k])
      if name not in p['sums']:      # num, den, saliency
        p['sums'][name] = torch.empty(3, self.N, self.H, self.W, dtype=torch.float32, device=self.device)
      if name not in p['scores'] or p['scores'][name].shape[0] != M:
        p['scores'][name] = torch.empty(M, self.N, dtype=torch.float32, device=self.device)
    return p

  def _perturb_head_weights(self, heads):
    """w_j of the prediction score: 1 on the columns of the selected heads (names as ``LSTMDecoder.select_loss_heads`` takes them)."""
    picked = resolve_heads(self.decoder.heads, heads)
    return [1.0 if k in picked else 0.0 for _, k, size, _, _ in self.decoder.heads for _ in range(size)]

  def perturbation_attributions(self, method, patch=None, stride=None, grid=7, keep_prob=0.5, steps=64, fill=None, score='prediction',
                                heads=None, seed=0, inputs=None):
    """Which pixels move the command when they are hidden: occlusion sensitivity or RISE on the batch ``load_batch`` left in the
    model.  Gradient-free: forwards only, on a model of any ``training``.

    ``method='occlusion'``: a hard ``patch`` = (ph, pw) (or one integer; None: a quarter of the image each way, rounded up) slides
    over a grid of ``stride`` = (sy, sx) (None: half the patch, rounded up); along y there are Gy = 1 positions if ph >= H, else
    ceil((H - ph) / sy) + 1, position j starts at min(j * sy, H - ph) (the last is clamped: every pixel is covered); step
    m = j * Gx + i, M = Gy * Gx.  The same patch for every sample; one larger than the image is clipped to it.  ``steps`` is not read.
    ``method='rise'``: M = ``steps`` random smooth masks per sample: (``grid`` + 1)^2 keep-bits, each kept with ``keep_prob``, shifted
    by a random offset within a cell and interpolated bilinearly (include/geeco_hip.h states the draws and the arithmetic), from the
    device's counter-based generator under ``seed`` (key: ``attribution.input_key`` of the pass's first input).  Not the original's
    estimator: RISE weights the KEPT mask by a class probability; a regression controller has no class score, so the weight here
    is the hidden share times the command's change, the same estimator as the occlusion grid.
    ``score='prediction'`` (no labels): d_m[n] = sum_j w_j (p_m[n][j] - p_0[n][j])^2 over the columns of ``decoder.preds``, w_j = 1
    on the columns of ``heads`` (None: all heads), p_0 the clean predictions.  ``score='loss'`` (signed): d_m[n] = loss_n(x_m) -
    loss_n(x) from ``LSTMDecoder.sample_losses``, of the loss of ``heads`` (None: the training loss); ValueError where the decoder
    keeps no per-sample terms or the batch came without labels.
    ``fill``: what a hidden pixel shows.  None = black; a [C] colour; a [H][W][C] frame; an array shaped like the input; or a dict of
    those by input name.  One array stands for 'rgb' (and 'target_rgb' when it fits); depth takes a fill through the dict form only.
    ``inputs``: the passes to run, by their first input: 'rgb' (the observation frames, and 'depth' with the same occluder -- the
    camera delivers both) and, for goal models, 'target_rgb' (+ 'target_depth'); None = every pass the model has.

    Returns a dict of device tensors: 'saliency' [N][H][W] -- ONE map per window, not per frame as the gradient methods give: the
    occluder is shared by the K frames of a window, as an object in front of the camera would be; 'coverage' [N][H][W] = sum_m o_m;
    'scores' [M][N]; for occlusion 'patch_scores' [Gy][Gx][N], a view of the scores; for goal models the same under
    'saliency_target', 'coverage_target', 'scores_target', 'patch_scores_target'; and 'predictions': the clean predictions by key.
    All of them are views of the pass's own buffers, which the next call on this model writes again: clone what must outlive it
    (``Estimator.perturbation_attributions`` copies to the host per batch).

    Refuses ``shared_frames`` and inputs bound as window addresses (``check_perturbation_attributions``).  Eager launches only; no
    host synchronisation and no allocation inside the loop (the buffers are made by the first call with these arguments);
    parameters, optimiser state and the step counter are only read.  Afterwards the model holds the clean inputs again, bit for
    bit, and the forward at them."""
    self.check_perturbation_attributions()
    check_perturbation_arguments(method, patch, stride, grid, keep_prob, steps, score, seed)
    have = [name for name in PASSES if name in self.inputs]
    passes = have if inputs is None else [inputs] if isinstance(inputs, str) else list(inputs)
    if not passes or set(passes) - set(have) or len(set(passes)) != len(passes):
      raise ValueError('perturbation_attributions: inputs=%r; the passes of this model are %s' % (inputs, ', '.join(repr(n) for n in have)))
    H, W, d = self.H, self.W, self.decoder
    occlusion = method == 'occlusion'
    if occlusion:
      ph, pw = _pair(patch) if patch is not None else (-(-H // 4), -(-W // 4))
      sy, sx = _pair(stride) if stride is not None else (-(-int(ph) // 2), -(-int(pw) // 2))
      descs = {name: ops.perturb_desc('occlusion', H, W, patch=(ph, pw), stride=(sy, sx)) for name in passes}
      Gy, Gx, _ = ops.perturb_patch(descs[passes[0]])
      M = Gy * Gx
    else:
      descs = {name: ops.perturb_desc('rise', H, W, grid=grid, keep_prob=keep_prob, key=input_key(seed, name)) for name in passes}
      M = int(steps)
    w = self._perturb_head_weights(heads)      # (checks ``heads`` for either score)
    by_loss = score == 'loss'
    if by_loss:
      if self.labels_missing is None or self.labels_missing:
        raise ValueError("perturbation_attributions: score='loss' needs the labels; the batch was loaded without %s (load_batch(features, "
                         "labels)); score='prediction' needs none" % (', '.join(self.labels_missing or self.label_keys),))
    selected = d.head_weights
    try:
      if by_loss:
        d.select_loss_heads(heads)
      out, preds0 = self._perturbation_pass(passes, descs, M, (Gy, Gx) if occlusion else None, fill, w, by_loss)
    finally:      # score='loss' with ``heads``: the last forward is the model's own again, its losses the ones it had
      d.head_weights = selected
    self.forward()      # the model holds the forward at the clean inputs again
    out['predictions'], off = {}, 0
    for _, key, size, _, _ in d.heads:
      out['predictions'][key] = preds0[:, off:off + size]
      off += size
    return out

  def _perturbation_pass(self, passes, descs, M, grid_shape, fill, w, by_loss):
    d = self.decoder
    p = self._perturb_buffers(passes, M)
    keys = [k for name in passes for k in PASSES[name] if k in self.inputs]
    # None (black) or per occluded input a [C] colour, a [H][W][C] frame or an array shaped like the input
    fills = periodic_operands(self, 'perturbation_attributions', 'fill', fill, keys,
                              lambda k: (tuple(self.inputs[k].shape), tuple(self.inputs[k].shape[-3:]), tuple(self.inputs[k].shape[-1:])), p['fill'],
                              known=[k for ks in PASSES.values() for k in ks if k in self.inputs])
    if by_loss:
      if d.sample_loss_terms() is None:
        raise ValueError("perturbation_attributions: score='loss' needs the decoder's per-sample loss terms, which this one does not keep "
                         "(LSTMDecoder.sample_losses: dim_h_fc outside {64, 128}, dim_h_lstm > 128, more than 32 outputs, loss_shaping "
                         "or the one-launch decoder); use score='prediction'")
    else:
      p['w'].copy_(torch.tensor(w, dtype=torch.float32), non_blocking=True)
    self.forward()      # the clean input: p_0, loss_n(x)
    p['preds0'].copy_(d.preds)
    if by_loss:
      d.sample_losses_into(p['losses'][0])
    out = {}
    for name in passes:
      desc, scores = descs[name], p['scores'][name]
      num, den, sal = p['sums'][name]
      group = [k for k in PASSES[name] if k in self.inputs]
      with clean_inputs(self, group, p['clean']):
        for m in range(M):
          for k in group:      # occlusion: only the previous patch and the step's own are written
            ops.perturb_apply_into(self.inputs[k], p['clean'][k], fills[k], desc, m, prev_step=m - 1 if grid_shape else -1)
          self.forward()
          if by_loss:
            d.sample_losses_into(p['losses'][1])
            p['losses'][1].sub_(p['losses'][0])
            scores[m].copy_(p['losses'][1])
          else:
            ops.perturb_score_into(scores[m], d.preds, p['preds0'], p['w'])
          ops.perturb_accumulate_into(num, den, scores[m], desc, m, overwrite=m == 0)
      ops.perturb_finish_into(sal, num, den)
      tail = '' if name == 'rgb' else '_target'
      out['saliency' + tail], out['coverage' + tail], out['scores' + tail] = sal, den, scores
      if grid_shape:
        out['patch_scores' + tail] = scores.view(grid_shape[0], grid_shape[1], self.N)
    return out, p['preds0']
