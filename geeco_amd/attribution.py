"""Integrated-gradients and SmoothGrad attributions on the device: ``_ModelBase.attributions``.

Both are "many input gradients along a family of perturbed inputs, summed".  The model's own forward, backward and input-gradient
pass run M times, untouched; what this module adds is the loop around them, on the device: the path point is written
into the model's own input buffers (csrc/attribution.hip: geeco_attr_path_point), each step's gradient goes into a running sum
(geeco_attr_accumulate), and one finish (geeco_attr_finish) forms the attributions, the saliency maps and the per-sample sums that
integrated gradients' completeness check reads.  Nothing is copied to the host inside the loop and nothing is allocated there.
"""
from __future__ import annotations

import numpy as np
import torch

from . import ops
from .attr_pass import check_steps_seed, clean_inputs, periodic_operands

IMAGE_KEYS = ('rgb', 'target_rgb', 'depth', 'target_depth')
METHODS = ('integrated_gradients', 'smoothgrad')


def input_key(seed, name):
  """The 64-bit Philox key of image input ``name`` under ``seed``: 4 * seed + the input's index in IMAGE_KEYS, so the inputs of one
  model draw independent noise (the counter of include/geeco_hip.h: geeco_attr_path_point holds the step and the element)."""
  return (4 * int(seed) + IMAGE_KEYS.index(name)) & ((1 << 64) - 1)


def check_attribution_arguments(method, steps, noise_std, seed):
  """ValueError, with the reason, for arguments no model serves."""
  if method not in METHODS:
    raise ValueError('attributions: method=%r must be one of %s' % (method, ', '.join(repr(m) for m in METHODS)))
  check_steps_seed('attributions', steps=steps)
  if not float(noise_std) >= 0.0 or not np.isfinite(float(noise_std)):
    raise ValueError('attributions: noise_std=%r must be a finite number >= 0' % (noise_std,))
  if method == 'integrated_gradients' and float(noise_std) != 0.0:
    raise ValueError("attributions: noise_std goes with method='smoothgrad' (integrated gradients follows the straight path)")
  check_steps_seed('attributions', seed=seed)


class Attributions:
  """The attribution pass of a model (mixed into ``graph._ModelBase``)."""

  _attr = None      # the pass's buffers, allocated by the first call

  def _attr_buffers(self):
    """Per image input: the clean copy, the running sum (which the finish turns into the attributions in place), the saliency map,
    the per-sample sums; for RGB-D the contiguous staging the 4-channel gradient is split into."""
    if self._attr is None:
      f32 = dict(dtype=torch.float32, device=self.device)
      keys = [k for k in IMAGE_KEYS if k in self.inputs]
      a = dict(keys=keys, clean={}, acc={}, saliency={}, sums={}, base={}, stage={}, losses=torch.zeros(2, **f32),
               sample_losses=torch.zeros(2, self.N, dtype=torch.float64, device=self.device))
      for k in keys:
        buf = self.inputs[k]
        a['clean'][k], a['acc'][k] = torch.empty_like(buf), torch.empty_like(buf)
        a['saliency'][k] = torch.empty(buf.shape[:-1], **f32)
        a['sums'][k] = torch.empty(self.N, **f32)
        if self.C == 4:
          a['stage'][k] = torch.empty_like(buf)
      self._attr = a
    return self._attr

  def _attr_gradient_sources(self, a):
    """The contiguous tensor per input that holds the step's gradient after ``input_gradients()``: the pass's own buffers for RGB
    models; for RGB-D the 4-channel buffers split into the staging tensors (the channel pack's adjoint, one launch each)."""
    HW = self.H * self.W
    if self.C == 3:
      src = {'rgb': self.d_frames}
      if self.goal:
        src['target_rgb'] = self.d_tgt
      return src
    st = a['stage']
    ops.pack_pixels_bwd_into(st['rgb'], self.d_frames, HW * 3, self.N * self.K, HW, 3, 4, d_src2=st['depth'], src2_sample_stride=HW, C2=1)
    if self.goal:
      ops.pack_pixels_bwd_into(st['target_rgb'], self.d_tgt, HW * 3, self.N, HW, 3, 4, d_src2=st['target_depth'], src2_sample_stride=HW, C2=1)
    return st

  def attributions(self, method, steps, baseline=None, noise_std=0.0, seed=0, chunk_frames=96):
    """Attributions of the loss to the image inputs of the batch ``load_batch`` left in the model.

    ``method='integrated_gradients'``: the midpoint rule over the straight path from ``baseline`` b to the input x, M = ``steps``
    points alpha_m = (m + 0.5) / M:  attr = (x - b) * (1 / M) sum_m d loss / d input (b + alpha_m (x - b)).  Its attributions sum to
    loss(x) - loss(b) up to the rule's error; 'completeness_gap' is what is missing.
    ``method='smoothgrad'``: attr = (1 / M) sum_m d loss / d input (x + noise_std * z_m), z_m ~ N(0, 1) per element from the
    device's counter-based generator under ``seed`` (key: ``input_key``; step m is the counter's step).  The noisy input is NOT
    clipped to [0, 1].
    ``baseline``: None = black; a [H][W][C] frame, broadcast over the frames; an array shaped like the input; or a dict of those by
    input name.  One array stands for 'rgb' (and 'target_rgb' when it is a frame or the shapes agree); depth inputs take a
    baseline through the dict form only, else black.  The target frame of a goal model follows the same rule as the observation
    frames, with its own baseline.

    Returns a dict of device tensors: per image input the attributions, shaped like the input; 'saliency' [N][K][H][W] and, for
    goal models, 'saliency_target' [N][H][W] = max_c |attr| of the rgb inputs; 'sample_sum' [N]: the sum of all attributions of a
    sample (fixed order; over every image input); 'loss': the loss at the clean input; and for integrated gradients
    'loss_baseline' and 'completeness_gap' [N] (float64) = sample_sum[n] - (loss_n(x) - loss_n(b)) per sample, loss_n = sample n's
    share of the batch-mean loss that is differentiated (``LSTMDecoder.sample_losses``: the per-sample loss terms the heads kernel
    leaves in its workspace on every forward; the L2 term has no share and cancels).  Their sum is the batch's gap,
    sum_n sample_sum[n] - (loss(x) - loss(b)).  Where the decoder keeps no per-sample terms (``sample_losses`` says which shapes:
    dim_h_fc outside {64, 128}, dim_h_lstm > 128, ``loss_shaping``) 'completeness_gap' is that batch-level number alone, [1].
    The dynamic-image models (geeco-f, 'dyndiff') normalise each image by its own range, rng = max - min + 1e-6: on the path from
    a baseline that is constant in time the image's range goes to 0 with alpha and the normalised image does not, so the path is
    strongly curved near alpha -> 0 and the gap falls slowly with M there.  That is the method's behaviour on this model, not an
    error of the pass.

    Same refusals as ``input_gradients`` (``check_input_gradients``).  Eager launches only; no host synchronisation and no
    allocation inside the loop (the buffers are made by the first call); the optimiser is never called, and parameters, moments
    and the step counter are only read.  Afterwards the model holds the clean inputs again, bit for bit, and the forward at them
    (``predictions()``, ``loss``)."""
    self.check_input_gradients()
    check_attribution_arguments(method, steps, noise_std, seed)
    M, ig = int(steps), method == 'integrated_gradients'
    a = self._attr_buffers()
    keys = a['keys']
    # None (black) or per input a [H][W][C] frame, broadcast over the frames, or an array shaped like the input
    base = periodic_operands(self, 'attributions', 'baseline', baseline if ig else None, keys,
                             lambda k: (tuple(self.inputs[k].shape), tuple(self.inputs[k].shape[-3:])), a['base'])
    d = self.decoder

    def point(alpha, sigma, m):
      for k in keys:
        ops.attr_path_point_into(self.inputs[k], a['clean'][k], base[k], alpha, sigma, input_key(seed, k), m)

    with clean_inputs(self, keys, a['clean']):
      if ig:      # loss(baseline): the path point at alpha = 0 is the baseline itself
        point(0.0, 0.0, 0)
        self.forward()
        a['losses'][1:2].copy_(self.loss.reshape(1))
        d.sample_losses_into(a['sample_losses'][1])
      for m in range(M):
        point((m + 0.5) / M if ig else 1.0, 0.0 if ig else float(noise_std), m)
        self.forward(backward_too=True)
        self.backward()
        self.input_gradients(chunk_frames)
        for k, g in self._attr_gradient_sources(a).items():
          ops.attr_accumulate_into(a['acc'][k], g, 1.0 / M, overwrite=m == 0)
    self.forward()      # the clean input's loss and predictions
    a['losses'][0:1].copy_(self.loss.reshape(1))
    per_sample = d.sample_losses_into(a['sample_losses'][0])
    out = {}
    for k in keys:
      shape = self.inputs[k].shape
      frames = 1 if k.startswith('target') else self.K
      ops.attr_finish_into(a['acc'][k], a['saliency'][k], a['sums'][k], a['acc'][k], a['clean'][k], base[k], ig, self.N, frames,
                           self.H * self.W, int(shape[-1]))
      out[k] = a['acc'][k]
    out['saliency'] = a['saliency']['rgb']
    if self.goal:
      out['saliency_target'] = a['saliency']['target_rgb']
    out['sample_sum'] = torch.stack([a['sums'][k] for k in keys]).sum(dim=0) if len(keys) > 1 else a['sums'][keys[0]]
    out['sample_sum_by_input'] = {k: a['sums'][k] for k in keys}
    out['loss'] = a['losses'][0]
    if ig:
      out['loss_baseline'] = a['losses'][1]
      if per_sample:
        out['completeness_gap'] = out['sample_sum'].double() - (a['sample_losses'][0] - a['sample_losses'][1])
      else:      # no per-sample loss terms for this decoder shape: the batch's gap
        out['completeness_gap'] = (out['sample_sum'].double().sum() - (a['losses'][0].double() - a['losses'][1].double())).reshape(1)
    return out
