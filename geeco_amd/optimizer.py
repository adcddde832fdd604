"""The optimiser step of the training models (estimator.py:243-244), ONE path behind every option: ``OptimizerStep`` is the part of
``graph._ModelBase`` that owns the optimiser's device scalars and runs Adam over the arena or pieces of it -- plain, with averaged weights
(DESIGN 5.15), behind the global norm of the gradient (5.16, 5.19), under a schedule (5.18), with per-scope multipliers (5.20).  The host
class provides ``cfg``, ``store``, ``device``, ``shared_frames``, the checked options (``options``) and ``_refresh_after_update()``."""
from __future__ import annotations

import numpy as np
import torch

from . import ops
from .train_options import check_exclusions
from .variables import backward_cut, lr_multiplier_runs, variable_stats_scalars


class OptimizerStep:
  def _setup_optimizer(self, training):
    """The options' attributes, from the record ``self.options`` (train_options.TrainOptions; None = the option is off), and the
    optimiser's state on the device, once the store exists."""
    f32 = dict(dtype=torch.float32, device=self.device)
    o = self.options
    check_exclusions(o, shared_frames=self.shared_frames is not None)
    # skip_limit: the consecutive skipped steps the caller tolerates.  grad_accum (5.23): A micro-batches per optimiser
    # step; the store then carries the accumulator (``_keep_accumulator``, once the decoder exists)
    self.ema_decay, self.clip_norm, self.skip_limit, self.lr_schedule = o.ema_decay, o.clip_norm, o.skip_limit, o.lr_schedule
    self.lr_multipliers, self.variable_stats_mode, self.loss_shaping, self.grad_accum = o.lr_multipliers, o.variable_stats_mode, o.loss_shaping, o.grad_accum
    # lr_schedule: the normalised schedule, and the struct the prepare work is handed in place of cfg.lr
    # (_prepare_args, _prepare_unless_done); the device then leaves lr(s) of the step in scal[2].  None: cfg.lr, as ever.
    self._lr_arg = float(self.cfg.lr) if self.lr_schedule is None else ops.lr_schedule_struct(self.lr_schedule)
    # lr_multipliers: the optimiser step is made of ``lr_runs``, the arena's maximal contiguous runs (offset, count,
    # multiplier) of one multiplier each with the frozen ones left out, and the backward stops at ``backward_cut``, the lowest layer
    # with anything to train.  None / 'full': the model without the option.
    self.lr_runs, self.backward_cut = None, 'full'
    if self.lr_multipliers is not None:
      self.lr_runs = lr_multiplier_runs(self.store.offsets, self.store.size, self.lr_multipliers)
      if not self.lr_runs:
        raise ValueError('lr_multipliers freezes every variable: there is nothing to train')
      if len(self.lr_runs) > ops._native.ADAM_SEGMENTS_MAX:
        raise ValueError('lr_multipliers: the table splits the arena into %d runs of one multiplier each; the optimiser step is one launch '
                         'over at most %d' % (len(self.lr_runs), ops._native.ADAM_SEGMENTS_MAX))
      self.backward_cut = backward_cut(self.lr_multipliers)
    self.scal = torch.zeros(4, **f32)          # [0] = Adam lr_t, [1] = sum of squares of the arena, [2] = lr(s) under lr_schedule
    self.world = 1
    self._prepared = False      # this step's backward has done adam_prepare's work (_prepare_args; runtime.py sets it too)
    # clip_norm: the sums of squares of the arena's chunks, [s, norm] of the last optimiser step, and the calls of
    # apply_gradients_of whose update waits for the norm of all of them; a model without the option has none of it.
    # skip_nonfinite shares them -- the norm decides whether the step is applied -- and adds ``guard``: int64 [verdict
    # of the last step (1 applied, 0 skipped), skipped steps in all, skipped steps in a row]
    self.clip_ws = self.clip_out = self.guard = None
    self._clip_calls = []
    if (self.clip_norm is not None or self.skip_limit is not None) and training:
      self.clip_ws = torch.zeros(ops.clip_ws_floats(self.store.size), **f32)
      self.clip_out = torch.zeros(2, **f32)
      if self.skip_limit is not None:
        self.guard = torch.zeros(3, dtype=torch.int64, device=self.device)
    # variable_stats: the chunk table, the workspace and the records of the statistics pass, and ``step_pieces``, where
    # the gradient of the step that ran last lives: the pieces (gradient source, offset, count) its optimiser step was handed.  A
    # replayed step runs no python, but its pieces are the ones recorded at capture.  A model without the option has none of it.
    self.stats_plan, self.step_pieces, self._open_pieces = None, None, []
    if self.variable_stats_mode is not None:
      s = self.store
      self.stats_plan = ops.VariableStatsPlan([(s.offsets[n], int(np.prod(s.shapes[n]))) for n in s.shapes], self.device)

  def _prepare_args(self, adam_prepare):
    """backward(adam_prepare=True): the step counter / lr_t update rides in the backward's last slab-sum launch (one dependent
    launch less); apply_gradients() then skips its own adam_prepare.  Only callers that DO apply the gradients next pass it
    (train_step, runtime.TrainStepRunner): the counter must advance exactly once per optimiser step."""
    if not adam_prepare:
      return None
    self._prepared = True
    return (self.store.global_step, self._lr_arg, self.scal)

  def _prepare_unless_done(self, last=True):
    """adam_prepare unless this step's backward carried it; ``last``: the optimiser step is complete behind this piece."""
    if not self._prepared:
      if self.lr_schedule is None:
        ops.adam_prepare(self.store.global_step, self._lr_arg, self.scal)
      else:
        ops.adam_prepare_schedule(self.store.global_step, self._lr_arg, self.scal)
    self._prepared = not last

  def _pieces(self, segments):
    """``segments`` as [(gradients, offset, count, multiplier)].  Under ``lr_multipliers`` they are intersected with ``lr_runs``: every
    piece then lies in one run and takes its multiplier, and what is frozen is in no piece, neither read nor written."""
    if self.lr_runs is None:
      return [(g, off, n, None) for g, off, n in segments]
    pieces = []
    for g, off, n in segments:
      for lo, cnt, mul in self.lr_runs:
        a, b = max(off, lo), min(off + n, lo + cnt)
        if a < b:
          pieces.append((g[a - off:b - off], a, b - a, mul))
    return pieces

  def _check_piece_count(self, n, what):
    if n > ops._native.ADAM_SEGMENTS_MAX:
      option = ' with '.join(o for o, on in (('clip_norm / skip_nonfinite', self.clip_ws is not None), ('lr_multipliers', self.lr_runs is not None)) if on)
      raise ValueError('%s: %s came in %d pieces; one launch takes at most %d' % (option, what, n, ops._native.ADAM_SEGMENTS_MAX))

  def _total_gradient_kw(self):      # the total gradient the update and the norm are formed of: g / world + l2 * p
    # (grad_accum_steps: g is the sum over the A micro-batches, so g / (world A) is the mean of their gradients and l2 * p is added once)
    return dict(grad_scale=1.0 / (self.world * (self.grad_accum or 1)), l2=float(self.cfg.l2_regularizer))

  def _launch_update(self, pieces, g_out, whole=False):
    """One launch of the Adam kernel over ``pieces`` (nothing for a call whose pieces are all frozen), through the entry point the model's
    options name; ``whole``: the one piece is the arena."""
    if not pieces:
      return
    s, kw = self.store, self._total_gradient_kw()
    segs = [q[:3] for q in pieces]
    ema = dict(ema=s.ema, global_step=s.global_step, decay=self.ema_decay) if s.ema is not None else {}      # the averaged weights follow in the same launch
    if self.lr_runs is not None:
      ops.adam_tf_segments_scaled(s.params, s.adam_m, s.adam_v, segs, [q[3] for q in pieces], self.scal, clip_dev=self.clip_out, guard=self.guard,
                                  g_out=g_out, **ema, **kw)
    elif self.guard is not None:
      ops.adam_tf_segments_guard(s.params, s.adam_m, s.adam_v, segs, self.scal, self.clip_out, self.guard, g_out=g_out, **ema, **kw)
    elif self.clip_ws is not None:
      ops.adam_tf_segments_clip(s.params, s.adam_m, s.adam_v, segs, self.scal, self.clip_out, g_out=g_out, **ema, **kw)
    elif whole and s.ema is not None:
      ops.adam_tf_ema(s.params, segs[0][0], s.adam_m, s.adam_v, s.ema, s.size, self.scal, s.global_step, self.ema_decay, **kw)
    elif whole:
      ops.adam_tf(s.params, segs[0][0], s.adam_m, s.adam_v, s.size, self.scal, **kw)
    elif s.ema is not None:
      ops.adam_tf_segments_ema(s.params, s.adam_m, s.adam_v, s.ema, segs, self.scal, s.global_step, self.ema_decay, g_out=g_out, **kw)
    else:
      ops.adam_tf_segments(s.params, s.adam_m, s.adam_v, segs, self.scal, g_out=g_out, **kw)

  def apply_gradients_of(self, segments, g_out=None, last=True):
    """The optimiser step of SOME pieces of the arena (data parallel: everything that came with the early bucket first, the late
    bucket's variables when it has arrived).  ``last``: the pieces complete the step (weight copies are re-derived behind it).
    One launch per call that has anything trainable.
    Under ``clip_norm`` and / or ``skip_nonfinite`` no piece may move before the norm of ALL of them is known, so the pieces of a call that
    does not complete the step are recorded and nothing is launched for them; the call that does runs, in order, the sum of squares
    over every recorded piece and its own (ONE launch: the partial sums are then bitwise those of the undivided arena, whatever the
    pieces), the scale, and the update call by call (each with its own ``g_out``).  Three launches for the whole arena, four for the
    two pieces of the schedules in runtime.py -- constant per schedule, so the step stays one captured graph.  Under ``skip_nonfinite``
    the scale comes from ``guard_decide`` (clip 0 = no clipping) with the verdict on the step, and the update is the one that honours it:
    the same launches whether the step is applied or skipped.  Under ``lr_multipliers`` the sum of squares gets the trainable pieces: the
    global norm is that of the trainable variables' gradients (tf.clip_by_global_norm over var_list), and a NaN in a frozen variable's
    gradient slot cannot cause a skip."""
    self._optimizer_step(segments, g_out, last)

  def _optimizer_step(self, segments, g_out, last, whole=False):
    pieces = self._pieces(segments)
    if self.stats_plan is not None:
      self._open_pieces += [q[:3] for q in pieces]
      if last:
        self.step_pieces, self._open_pieces = self._open_pieces, []
    if self.clip_ws is None:      # nothing to wait for
      if self.lr_runs is not None:      # (without the option ops.adam_tf_segments refuses the count)
        self._check_piece_count(len(pieces), 'one call of the optimiser step')
      self._prepare_unless_done(last)
      self._launch_update(pieces, g_out, whole)
    else:
      self._clip_calls.append((pieces, g_out))
      if not last:
        return
      s, calls, self._clip_calls = self.store, self._clip_calls, []
      every = [q[:3] for ps, _ in calls for q in ps]
      self._check_piece_count(len(every), 'the optimiser step')      # the norm of the whole gradient is one launch
      self._prepare_unless_done()
      ops.grad_sumsq_segments(self.clip_ws, s.params, every, s.size, **self._total_gradient_kw())
      if self.guard is not None:
        ops.guard_decide(self.clip_out, self.guard, self.clip_ws, self.clip_ws.numel(), self.clip_norm or 0.0)
      else:
        ops.clip_scale(self.clip_out, self.clip_ws, self.clip_ws.numel(), self.clip_norm)
      for ps, out in calls:
        self._launch_update(ps, out)
    if last:
      self._refresh_after_update()

  def apply_gradients(self):
    """The whole arena through the same path: the one-piece call (under ``lr_multipliers``: the runs themselves)."""
    del self._clip_calls[:]
    del self._open_pieces[:]
    self._optimizer_step([(self.gradient_source(), 0, self.store.size)], None, True, whole=True)

  # -- gradient accumulation over micro-batches -----------------------------------
  def _keep_accumulator(self):
    """Once the decoder exists: the store's accumulator and loss buffers (shared with every model built on the store)."""
    if self.grad_accum is not None:
      self.store.keep_accumulator(self.decoder.losses.numel())

  def gradient_source(self):
    """The arena the optimiser step reads: the gradients of this batch, or under ``grad_accum_steps`` their sum over the group."""
    return self.store.grads if self.grad_accum is None else self.store.accum

  def micro_step_form(self):
    """The form of the next micro-step, from the store's count of accumulated micro-batches: 'first' (the accumulator is overwritten),
    'middle' (added to), 'last' (added to, then the optimiser step on the accumulator); None for a model without the option."""
    if self.grad_accum is None:
      return None
    c = self.store.accum_count
    return 'first' if c == 0 else 'last' if c == self.grad_accum - 1 else 'middle'

  def micro_step_done(self, form):
    """Advances the store's count behind a micro-step of ``form``; True when that micro-step applied the optimiser step."""
    self.store.accum_count = 0 if form == 'last' else self.store.accum_count + 1
    return form == 'last'

  def accumulate_gradients_of(self, segments, overwrite):
    """One launch: the pieces of ``segments`` (as apply_gradients_of takes them, under ``lr_multipliers`` cut down to what is trained:
    a frozen variable is neither read nor accumulated) stored into (``overwrite``) or added to ``store.accum``."""
    pieces = [q[:3] for q in self._pieces(segments)]
    if not pieces:
      return
    if len(pieces) > ops._native.ADAM_SEGMENTS_MAX:
      raise ValueError('grad_accum_steps: one call of the accumulate launch came in %d pieces; one launch takes at most %d'
                       % (len(pieces), ops._native.ADAM_SEGMENTS_MAX))
    ops.grad_accumulate_segments(self.store.accum, pieces, self.store.size, overwrite)

  def _accumulate_losses(self, form):
    """The loss terms of this micro-batch into the store's sum, and behind the group's last one their mean: tensor work on the
    stream (captured with the micro-step), no host read."""
    s, l = self.store, self.decoder.losses
    if form == 'first':
      s.accum_loss_sum.copy_(l)
    else:
      s.accum_loss_sum.add_(l)
    if form == 'last':
      torch.mul(s.accum_loss_sum, 1.0 / self.grad_accum, out=s.accum_loss_mean)

  # -- per-variable statistics ---------------------------------------------------
  def variable_stats(self):
    """{variable name: dict} of the step that ran last (``variables.variable_stats_scalars``: grad_norm, grad_max_abs, grad_mean,
    grad_zero_fraction, grad_nonfinite, weight_norm, weight_max_abs, weight_nonfinite, update_norm, update_ratio, and 'histograms'
    under ``variable_stats='histograms'``).  Two launches on the current stream, eagerly, then the records, lr_t and the verdict are
    READ: the call synchronises, so it belongs where the host waits anyway (the logging hook), never inside a captured step."""
    if self.stats_plan is None:
      raise RuntimeError("variable_stats(): the model was built without variable_stats (params['variable_stats'])")
    if not self.step_pieces:
      raise RuntimeError('variable_stats(): no optimiser step has run yet')
    s = self.store
    if len(self.step_pieces) > ops._native.ADAM_SEGMENTS_MAX:
      raise ValueError('variable_stats: the gradient of the last step came in %d pieces; one launch takes at most %d'
                       % (len(self.step_pieces), ops._native.ADAM_SEGMENTS_MAX))
    self.stats_plan.run(s.params, s.adam_m, s.adam_v, self.step_pieces, s.size, grad_scale=self._total_gradient_kw()['grad_scale'])
    recs = self.stats_plan.records()
    lr_t = float(self.scal[0])
    applied = True if self.guard is None else bool(int(self.guard[0]))
    out = {}
    for rec, name in zip(recs, s.shapes):
      mul = 1.0 if self.lr_multipliers is None else self.lr_multipliers[name]
      out[name] = variable_stats_scalars(rec, int(np.prod(s.shapes[name])), lr_t, mul, applied, self.variable_stats_mode == 'histograms')
    return out

  def nonfinite_gradient_variables(self, stats=None):
    """{variable name: number of non-finite gradient elements} of the step that ran last, the variables with none left out."""
    stats = self.variable_stats() if stats is None else stats
    return {n: d['grad_nonfinite'] for n, d in stats.items() if d['grad_nonfinite']}
