"""The LSTM decoder with its heads and losses: ``head_table`` and ``LSTMDecoder`` (``lstm_decoder`` and the loss functions, the
reference's graph.py:198-260, 430-500; estimator.py:206-239)."""
from __future__ import annotations

import torch

from . import _native, ops
from .variables import VariableStore


def head_table(cfg, loss_shaping=None):
  """(variable name, prediction key, size, kind, loss weight) per head, in variable creation order.
  kind 0 = mean_squared_error, 1 = softmax cross-entropy (graph.py:233-259, 430-500; estimator.py:224-237); 2 = huber_loss for the
  regression heads ``loss_shaping['huber_delta']`` (``train_options.check_loss_shaping``'s result) names."""
  if cfg.control_mode == 'cartesian':
    lam = float(cfg.lambda_aux)
    heads = [('pred_cmd_ee', 'cmd_ee', 3, 0, 1.0), ('logits_cmd_grp', 'logits_cmd_grp', cfg.num_grp_states, 1, 1.0),
             ('pred_aux_ee', 'pos_ee', 3, 0, lam), ('pred_aux_obj', 'pos_obj', 3, 0, lam)]
  elif cfg.control_mode == 'velocity':   # mse_loss sums all five terms unweighted (graph.py:446-449)
    heads = [('pred_cmd_vel', 'cmd_vel', cfg.dim_jnt_state, 0, 1.0), ('pred_cmd_ee', 'cmd_ee', 3, 0, 1.0),
             ('pred_cmd_grp', 'cmd_grp', cfg.dim_grp_command, 0, 1.0), ('pred_aux_ee', 'pos_ee', 3, 0, 1.0),
             ('pred_aux_obj', 'pos_obj', 3, 0, 1.0)]
  else:
    raise ValueError("Unknown control mode '%s'" % (cfg.control_mode,))
  huber = (loss_shaping or {}).get('huber_delta') or {}
  return [(name, key, size, 2 if kind == 0 and key in huber else kind, w) for name, key, size, kind, w in heads]


def resolve_heads(table, heads):
  """The prediction keys of the heads ``heads`` names in the head table ``table`` (rows (variable, key, size, kind, weight)): one
  name or several, 'logits_cmd_grp' also as 'cmd_grp'; None = every head.  ValueError for an empty selection or an unknown name."""
  keys = [h[1] for h in table]
  short = {k.replace('logits_', ''): k for k in keys}
  picked = set(keys) if heads is None else {short.get(h, h) for h in ([heads] if isinstance(heads, str) else heads)}
  if not picked or picked - set(keys):
    raise ValueError('heads=%r: this model has the heads %s' % (heads, ', '.join(sorted(short))))
  return picked


class LSTMDecoder:
  """T LSTM steps over states [T][N][D] from a zero state, fc1 + heads on the last output."""

  def __init__(self, store: VariableStore, scope, cfg, N, T, D, training, one_launch=False, loss_shaping=None):
    """``loss_shaping`` (``train_options.check_loss_shaping``'s result, None = off): the losses and their gradients come from the shaped
    entry points; with ``sample_weights`` the model binds ``sample_weight`` [N] beside the targets.
    ``one_launch`` (inference decoders with T > 1 only; the batched predictor engine sets it): forward(False) is the hoisted
    input projection + ONE launch for the T steps, fc1 and the heads (ops.lstm_seq_heads_into).  No per-step gates / c / h history
    is kept, no loss terms are computed and ``targets`` are not read; ``losses`` stays zero."""
    self.store, self.scope, self.cfg, self.N, self.T, self.D = store, scope, cfg, N, T, D
    self.H, self.F, self.training = cfg.dim_h_lstm, cfg.dim_h_fc, training
    self.one_launch = bool(one_launch) and not training and T > 1
    self.loss_shaping = loss_shaping
    self.heads = head_table(cfg, loss_shaping)
    self.OT = sum(h[2] for h in self.heads)
    f32 = dict(dtype=torch.float32, device=store.device)
    H = self.H
    self.states = torch.empty(T, N, D, **f32)
    self.preds = torch.empty(N, self.OT, **f32)
    self.losses = torch.zeros(8, **f32)
    if self.one_launch:
      self.zx = torch.empty(T, N, 4 * H, **f32)      # X Wx of all steps: all the one-launch kernel reads besides the weights
      self.z = self.gates = self.c = self.h = self.heads_ws = None
    else:
      self._alloc_chain()
    gemm_shapes = [(T * N, 4 * H, D), (N, 4 * H, H)]
    if training:
      self.dstates = torch.empty(T, N, D, **f32)
      self.dz = torch.empty(T, N, 4 * H, **f32)
      self.dh, self.dc = torch.empty(N, H, **f32), torch.empty(N, H, **f32)
      gemm_shapes += [(D, 4 * H, T * N), (H, 4 * H, max((T - 1) * N, 1)), (T * N, D, 4 * H), (N, H, 4 * H)]
    self.gemm_ws = torch.empty(max(ops.gemm_ws_bytes(*s) for s in gemm_shapes) // 4 + 4, **f32)
    self.targets, self.target_strides, self.loss_scale = None, None, 1.0     # bound by the model
    self.sample_weight, self.class_weight = None, None                      # loss_shaping: bound by the model; the table, made once
    if loss_shaping is not None and loss_shaping['grp_class_weights'] is not None:
      self.class_weight = torch.tensor(loss_shaping['grp_class_weights'], **f32)
    self.heads_pending, self.dz_from_heads = None, False
    self.head_weights = None      # select_loss_heads: the loss weights of an eager pass of its own; None = the table's (training)
    self._sample_loss_scratch = None      # sample_losses_into: made on first use

  def select_loss_heads(self, heads=None):
    """The loss this decoder differentiates from now on: the sum of the named heads' losses with weight 1, every other head 0
    (``heads``: head names of ``predictions()``, 'logits_cmd_grp' also as 'cmd_grp'); None = the training loss again.  The weights are
    the host ``head_weight`` array of every heads call, so a step captured into a graph keeps the ones it was captured with: this is
    for models that run eagerly and never train (``Estimator.input_gradients``)."""
    if heads is None:
      self.head_weights = None
      return
    picked = resolve_heads(self.heads, heads)
    self.head_weights = [1.0 if h[1] in picked else 0.0 for h in self.heads]

  def _alloc_chain(self):
    """The per-step buffers of the launch-per-step chain."""
    N, T, H = self.N, self.T, self.H
    f32 = dict(dtype=torch.float32, device=self.store.device)
    self.z = torch.empty(T, N, 4 * H, **f32)
    self.gates = torch.empty(T, N, 4 * H, **f32)
    self.c = torch.empty(T, N, H, **f32)
    self.h = torch.empty(T, N, H, **f32)
    self.heads_ws = torch.empty(ops.heads_ws_bytes(N, H, self.F) // 4 + 4, **f32)

  def _v(self, n):
    return self.store.var('%s/%s' % (self.scope, n))

  def _g(self, n):
    return self.store.grad('%s/%s' % (self.scope, n))

  def _weights(self):
    W = self._v('lstm_cell/kernel')            # [D + H][4H]: rows 0..D-1 multiply x, D.. multiply h
    return W[:self.D], W[self.D:], self._v('lstm_cell/bias')

  def _head_args(self, backward_too):
    """The head arguments of the ops (variables, sizes, kinds, loss weights, targets) and the gradient views, from the store as it is now."""
    names = [h[0] for h in self.heads]
    args = (self._v('fc1/kernel'), self._v('fc1/bias'), [self._v(n + '/kernel') for n in names], [self._v(n + '/bias') for n in names],
            [h[2] for h in self.heads], [h[3] for h in self.heads], self.head_weights or [h[4] for h in self.heads], self.targets,
            self.target_strides, float(self.loss_scale))
    grads = dict(d_fc1_w=self._g('fc1/kernel'), d_fc1_b=self._g('fc1/bias'), d_heads_w=[self._g(n + '/kernel') for n in names],
                 d_heads_b=[self._g(n + '/bias') for n in names]) if backward_too else {}
    if self.loss_shaping is not None:
      ls = self.loss_shaping
      if ls['sample_weights'] and self.sample_weight is None:
        raise RuntimeError("LSTMDecoder: loss_shaping['sample_weights'] is on but no sample_weight buffer is bound")
      grads['shaping'] = ops.loss_shaping(self.sample_weight if ls['sample_weights'] else None, self.class_weight, ls['label_smoothing'],
                                          [ls['huber_delta'].get(h[1], 0.0) for h in self.heads])
    return args, grads

  def forward(self, backward_too):
    args, grads = self._head_args(backward_too)
    self.heads_pending, self.dz_from_heads = None, False
    if self.one_launch and not backward_too:
      if self._forward_one_launch(args):
        return
      self.one_launch, self.zx = False, None      # sizes the kernel does not serve: today's chain from here on
      self._alloc_chain()
    if self.T == 1:
      self._forward_one_step(backward_too, args, grads)
    else:
      self._forward_chain(backward_too, args, grads)

  def _forward_one_launch(self, args):
    """Inference, T > 1: the hoisted input projection, then ONE launch for the T steps, fc1 and the heads (Wh register-resident,
    one workgroup per sample) instead of ~3 dependent launches per step.  False: the kernel does not serve these sizes."""
    N, T, D, H = self.N, self.T, self.D, self.H
    Wx, Wh, bias = self._weights()
    ops.gemm_into(self.zx, self.states, Wx, T * N, 4 * H, D, D, 4 * H, 4 * H, ws=self.gemm_ws)
    return ops.lstm_seq_heads_into(self.preds, self.zx, Wh, bias, *args[:5], N, T, H, self.F, 4 * H, 4 * H)      # (no losses: nothing to shape)

  def _forward_one_step(self, backward_too, args, grads):
    """One step from a zero state (round 5): gate GEMM + ONE per-sample launch for the slab sum, the gate math, fc1, the heads, the
    loss terms and (training) everything back to the gate gradients dz; the batch sums (weight / bias gradients, loss means) ride
    in the first grid of backward()'s launch pair -- losses / those gradients are final after backward()."""
    Wx, _, bias = self._weights()
    step = (self.z[0], self.c[0], self.h[0], self.gates[0], self.states[0], Wx, bias, self.N, self.H, self.D, self.D, 4 * self.H,
            self.gemm_ws)
    pend = _native.HeadsFinish() if backward_too else None
    if ops.lstm_step_heads_into(*step, self.preds, self.losses, *args, self.F, self.heads_ws,
                                dz=self.dz[0] if backward_too else None, pending=pend, **grads):
      self.heads_pending, self.dz_from_heads = pend, backward_too
      return
    # (shapes outside the fused step) the slab sum of the gate GEMM rides in the gate kernel (bitwise the same)
    ops.lstm_input_step_fwd_into(*step)
    self._heads_loss(backward_too, args, grads)

  def _forward_chain(self, backward_too, args, grads):
    N, T, D, H = self.N, self.T, self.D, self.H
    Wx, Wh, bias = self._weights()
    # hoisted input projection for all steps: Z = X Wx
    ops.gemm_into(self.z, self.states, Wx, T * N, 4 * H, D, D, 4 * H, 4 * H, ws=self.gemm_ws)
    for t in range(T):
      if t > 0:
        ops.gemm_into(self.z[t], self.h[t - 1], Wh, N, 4 * H, H, H, 4 * H, 4 * H, accumulate=True, ws=self.gemm_ws)
      ops.lstm_gates_fwd_into(self.c[t], self.h[t], self.gates[t], self.z[t], bias, self.c[t - 1] if t > 0 else None, N, H)
    self._heads_loss(backward_too, args, grads)

  def _heads_loss(self, backward_too, args, grads):
    kw = dict(dh=self.dh, **grads) if backward_too else dict(grads)      # (forward only: grads holds at most the shaping)
    ops.heads_loss_into(self.preds, self.losses, self.h[self.T - 1], *args, self.N, self.H, self.F, self.heads_ws, **kw)

  def backward(self, concat=None):
    """After forward(backward_too=True): fills d(states) and the LSTM variable gradients.  ``concat`` (one-step decoders
    only): dict(feats, dfeats, feat_ch, jnt_pos, J, cells) of the state concat that produced ``states``; its backward
    (feature gradients + ReluGrad of conv8) then rides in the same launch as the weight / input gradients and the method
    returns True (else the caller scatters ``dstates`` itself)."""
    N, T, D, H = self.N, self.T, self.D, self.H
    Wx, Wh, _ = self._weights()
    dW = self._g('lstm_cell/kernel')
    if T == 1:
      # one step from a zero state: dWh = h_prev^T dz = 0 (the arena's rows stay zero); weight / bias / input gradients (+ the
      # state-concat backward) in ONE launch instead of five dependent ones
      if not self.dz_from_heads:       # (the fused forward left dz itself)
        ops.lstm_gates_bwd_into(self.dz[0], None, self.gates[0], None, self.c[0], self.dh, None, N, H)
      kw = dict(feats_fwd=concat['feats'], dfeats=concat['dfeats'], feat_ch=concat['feat_ch'], jnt_pos=concat['jnt_pos'],
                J=concat['J'], cells=concat['cells']) if concat else {}
      ops.lstm_step_bwd_into(dW[:D], self._g('lstm_cell/bias'), self.dstates[0], self.states[0], self.dz[0], Wx, N, D, 4 * H,
                             4 * H, self.gemm_ws, pending=self.heads_pending, **kw)
      self.heads_pending = None
      return concat is not None
    for t in range(T - 1, -1, -1):
      ops.lstm_gates_bwd_into(self.dz[t], self.dc if t > 0 else None, self.gates[t], self.c[t - 1] if t > 0 else None, self.c[t],
                              self.dh, None if t == T - 1 else self.dc, N, H)
      if t > 0:   # dh_{t-1} = dz_t Wh^T
        ops.gemm_into(self.dh, self.dz[t], Wh, N, H, 4 * H, 4 * H, 4 * H, H, tb=True, ws=self.gemm_ws)
    # dWx = X^T dZ ; dWh = H_prev^T dZ[1:] ; db = colsum(dZ) ; dX = dZ Wx^T
    ops.gemm_into(dW[:D], self.states, self.dz, D, 4 * H, T * N, D, 4 * H, 4 * H, ta=True, ws=self.gemm_ws)
    ops.gemm_into(dW[D:], self.h, self.dz[1:], H, 4 * H, (T - 1) * N, H, 4 * H, 4 * H, ta=True, ws=self.gemm_ws)
    ops.colsum_into(self._g('lstm_cell/bias'), self.dz, 4 * H, T * N, 4 * H)
    ops.gemm_into(self.dstates, self.dz, Wx, T * N, D, 4 * H, 4 * H, 4 * H, D, tb=True, ws=self.gemm_ws)
    return False

  def sample_losses(self):
    """float64 [N]: each sample's share of the last forward's loss (no L2 term), so that their sum is ``losses[0]`` up to rounding --
    or None where the rows do not exist.  Every forward of the per-sample heads kernel (csrc/decoder_heads.hip: heads_sample_kernel,
    both the fused step and ``heads_loss_into``) leaves the raw loss term of sample n and head h at ``heads_ws[2 N F + 32 N + 32 F + 8 n
    + h]`` (HeadsParams::lterm): the sum of squared differences of a regression head, the cross-entropy of the gripper head; the
    finish role turns their batch sums into means (1 / (N size), 1 / N) and weights them, which is repeated here per sample.  None:
    the single-workgroup heads kernel wrote the losses (dim_h_fc outside {64, 128}, dim_h_lstm > 128 or more than 32 outputs: it
    keeps no rows), the one-launch inference decoder ran (no losses at all), or ``loss_shaping`` is on (the rows then hold weighted
    terms whose means are taken over batch-wide counts)."""
    out = torch.empty(self.N, dtype=torch.float64, device=self.preds.device)
    return out if self.sample_losses_into(out) else None

  def sample_losses_into(self, out):
    """``sample_losses`` into ``out`` (float64 [N]) without an allocation on the device: the rows widened into the decoder's own
    scratch, then one matrix-vector product with the coefficients (uploaded when they change: ``select_loss_heads``).  False, and
    ``out`` untouched, where the rows do not exist."""
    terms = self.sample_loss_terms()
    if terms is None:
      return False
    rows, coef = terms
    if self._sample_loss_scratch is None:      # (N and the head table are fixed per decoder: so are the two shapes)
      f64 = dict(dtype=torch.float64, device=rows.device)
      self._sample_loss_scratch = dict(rows=torch.empty(rows.shape, **f64), coef=torch.empty(len(coef), **f64), host=None)
    sc = self._sample_loss_scratch
    if sc['host'] != coef:
      sc['coef'].copy_(torch.tensor(coef, dtype=torch.float64), non_blocking=True)
      sc['host'] = coef
    sc['rows'].copy_(rows)
    torch.mv(sc['rows'], sc['coef'], out=out)
    return True

  def sample_loss_terms(self):
    """What ``sample_losses`` is made of: (the float32 view [N][heads] of the raw per-sample loss terms in the heads workspace -- it
    shows the last forward's, whenever it is read -- and each head's coefficient), or None where the rows do not exist."""
    N, F = self.N, self.F
    if self.loss_shaping is not None or self.one_launch or not (self.H <= 128 and F in (64, 128) and self.OT <= 32):
      return None
    off = 2 * N * F + 32 * N + 32 * F
    rows = self.heads_ws[off:off + 8 * N].view(N, 8)[:, :len(self.heads)]
    weights = self.head_weights or [h[4] for h in self.heads]
    return rows, [w / (N * size) if kind == 0 else w / N for (_, _, size, kind, _), w in zip(self.heads, weights)]

  def predictions(self):
    """The heads' slices of ``preds`` by prediction key (estimator.py:48-61 / 183-197)."""
    out, off = {}, 0
    for _, key, size, _, _ in self.heads:
      out[key] = self.preds[:, off:off + size]
      off += size
    return out
