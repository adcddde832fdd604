"""The grouped conv encoders: ``ConvEncoderStack`` owns the buffers, the launch plan and the backward schedule of the G encoders
of a model (``conv_encoder``, the reference's graph.py:61-117), every layer ONE launch over all groups."""
from __future__ import annotations

import torch

from . import ops
from .variables import ENC_FILTERS, ENC_STRIDES, VariableStore


def check_image_size(H, W):
  """Seven stride-2 layers must end on the hard-coded 2x2 grid of the joint state (graph.py:139)."""
  if (ops.same_out(H, 128), ops.same_out(W, 128)) != (2, 2):
    raise ValueError('the 2x2 state tiling needs 129..256 pixel inputs, got %dx%d' % (H, W))


class ConvEncoderStack:
  """``conv_encoder`` for G weight sets with identical shapes, Nf frames each."""

  # The data-parallel runner cuts the backward here: 'upper' = conv8 .. conv(SPLIT+1) down to that layer's filter gradient, 'bottom'
  # opens with its INPUT gradient and runs conv(SPLIT) .. conv1 (round 4 cut after it: every gradient of the early bucket exists once
  # that filter gradient does, so the bucket leaves a launch earlier)
  SPLIT = 2

  def __init__(self, store: VariableStore, scopes, Nf, H, W, Cin, dim_out, training):
    """``dim_out``: conv8's output channels, one int or one per encoder (dim_s_obs / dim_s_dyn / dim_s_diff,
    graph.py:390,394,402).  With unequal values conv1..conv7 still run as grouped launches and conv8 (the only layer
    whose shape differs) runs once per encoder (``split_top``)."""
    self.store, self.scopes, self.G, self.Nf = store, list(scopes), len(scopes), Nf
    self.Cin = Cin
    self.late = None       # (staging buffer, per-encoder length): see redirect_late_gradients
    # CUs the two persistent bottom-of-the-backward launches leave to a collective running beside them: a launch argument
    # (runtime.TrainStepRunner sets it around its own part 2, so every runner captures the grids it was built for)
    self.reserved_cus = 0
    self.dim_outs = [int(d) for d in dim_out] if isinstance(dim_out, (list, tuple)) else [int(dim_out)] * len(self.scopes)
    self.split_top = len(set(self.dim_outs)) > 1
    dim_out = max(self.dim_outs)
    # Backward schedule: ONE stream.  Round 1 ran the filter-gradient launches of the upper layers on two side streams
    # beside the input-gradient chain (+1-2 % then: the gather wgrad kernel left MFMA slack for its neighbour); with the
    # LDS-staged wgrad kernels every big launch fills the chip by itself and the two schedules measured the same (3.717 vs
    # 3.719 ms), so the side streams were retired (scripts/dev/SWITCHES.md).
    # conv7's + conv8's filter gradients and conv7's input gradient go into one grid (launch_top_bwd); bench.py reads
    # these two to label that row of its per-layer table
    self.pair_top = True
    self.hetero_top = 1
    self.derived_version = -1
    # Only the FIRST training stack built on a store may rely on the post-Adam refresh of its derived
    # weight copies; eval / predict stacks and any later training stack (e.g. the model built for a
    # ragged final batch) share the parameters but not the copies, so they re-derive on every forward.
    self.lazy_refresh = training and store.primary_stack is None
    if self.lazy_refresh:
      store.primary_stack = self
    self.Cpad = -(-Cin // 4) * 4
    self.training = training
    dev = store.device
    G = self.G
    # group stride inside the parameter arena (all encoders have the same shapes)
    if G > 1:
      gs = store.offsets[self.scopes[1] + '/conv1/kernel'] - store.offsets[self.scopes[0] + '/conv1/kernel']
      for g in range(G):
        for l in range(1, 8 if self.split_top else 9):
          for kind in ('kernel', 'bias'):
            a = store.offsets['%s/conv%d/%s' % (self.scopes[g], l, kind)]
            b = store.offsets['%s/conv%d/%s' % (self.scopes[0], l, kind)]
            if a - b != g * gs:
              raise ValueError('encoders are not uniformly strided in the arena')
    self.gs_p = gs if G > 1 else 0
    # layer geometry
    self.layers = []
    h, w, c = H, W, self.Cpad
    for l in range(8):
      cout = (list(ENC_FILTERS) + [dim_out])[l]
      s = ENC_STRIDES[l]
      ho, wo = ops.same_out(h, s), ops.same_out(w, s)
      self.layers.append(dict(H=h, W=w, Cin=c, Cout=cout, stride=s, Ho=ho, Wo=wo))
      h, w, c = ho, wo, cout
    self.out_hw = (h, w)
    f32 = dict(dtype=torch.float32, device=dev)
    self.x_in = torch.zeros(G, Nf, H, W, self.Cpad, **f32)
    self.acts = [torch.empty(G, Nf, L['Ho'], L['Wo'], L['Cout'], **f32) for L in self.layers]
    if self.split_top:      # per-encoder conv8 outputs of different widths
      L7 = self.layers[7]
      self.acts[7] = [torch.empty(Nf, L7['Ho'], L7['Wo'], d, **f32) for d in self.dim_outs]
    self.pad1 = self.Cpad != Cin
    self.pad1_copy = self.pad1      # the channel-padded copy of conv1's kernel is kept up to date (see below)
    if self.pad1:
      self.w1p = torch.zeros(G, 3, 3, self.Cpad, self.layers[0]['Cout'], **f32)
    # what only a training stack can have: False / empty / None on every other one
    self.fused_bottom = self.relu_bits = self.relu_fields = self.relu_fields3 = False
    self.bits1 = self.fields2 = self.fields3 = None      # the signs of conv1's / conv2's / conv3's outputs, for the backward
    self.needs_wt, self.needs_wt7, self.sides = [False] * 8, [], []      # (needs_wt7: conv8 per encoder, split_top)
    if training:
      # encoder bottom fused backward (conv2 dgrad + conv1 wgrad): the reference encoder's shapes, even sizes
      L0, L1 = self.layers[0], self.layers[1]
      self.fused_bottom = (self.Cpad == 4 and self.Cin in (3, 4) and L0['Cout'] == 32 and L0['stride'] == 1
                           and L1['Cout'] == 48 and L1['stride'] == 2 and L1['H'] % 2 == 0 and L1['W'] % 2 == 0)
      # the fused bottom only needs the SIGN of conv1's output (ReluGrad): conv1's forward writes one bit word per pixel
      # next to y1 and the backward reads those 25 MB instead of the 805 MB of y1
      self.relu_bits = self.fused_bottom
      # with the fused bottom and the sign bits nothing reads the channel-padded copy of conv1's kernel any more: conv1's
      # forward takes the RGB variable itself (together with the gather GEMM reading HWIO kernels this leaves NO weight
      # copy to re-derive after Adam: one launch less per step)
      if self.relu_bits and self.Cin == 3:
        self.pad1_copy = False
      if self.relu_bits:
        self.bits1 = torch.zeros(G, Nf, ops.relu_bits_rows(L0['H']), ops.relu_bits_pitch(L0['W']), dtype=torch.int32, device=dev)
      # the same one layer up: conv2's forward leaves 16-bit sign fields of y2 for conv3's input-gradient kernel
      L2 = self.layers[2]
      self.relu_fields = ((L1['Cin'], L1['Cout'], L1['stride']) == (32, 48, 2)
                          and (L2['Cin'], L2['Cout'], L2['stride']) == (48, 64, 2)
                          and L1['H'] % 2 == 0 and L1['W'] % 2 == 0 and L2['H'] % 2 == 0 and L2['W'] % 2 == 0)
      if self.relu_fields:
        self.fields2 = torch.zeros(G, ops.relu_fields_elems(Nf, L2['H'], L2['W']), dtype=torch.int16, device=dev)
      # ... and conv3's forward leaves byte sign fields of y3 for conv4's LDS-staged input-gradient kernel
      L3 = self.layers[3]
      self.relu_fields3 = (self.relu_fields and L3['Cin'] == 64
                           and L3['stride'] == 2 and ops.conv3x3_dgrad_relu_fields_supported(L3['H'], L3['W'], L3['Cin'], L3['Cout'], 2))
      if self.relu_fields3:
        self.fields3 = torch.zeros(G, Nf, L3['H'], L3['W'], L3['Cin'] // 8, dtype=torch.uint8, device=dev)
      # dz[0] (conv1's pre-activation gradient, the largest tensor of the step) never exists when the bottom is fused
      self.dz = [None if (i == 0 and self.fused_bottom) else
                 ([torch.empty_like(t) for t in a] if isinstance(a, list) else torch.empty_like(a)) for i, a in enumerate(self.acts)]
      # per-tap transposed kernel copies exist ONLY for the layers whose input-gradient kernel reads them (none in the bench
      # shapes: the LDS-staged kernels and the gather GEMM read the HWIO kernel); every other layer passes wt = NULL, so
      # a dispatcher that disagreed with geeco_conv3x3_dgrad_needs_wt would fail its null-pointer check, not read garbage
      self.needs_wt = [False] + [ops.conv3x3_dgrad_needs_wt(L['H'], L['W'], L['Cin'], L['Cout'], L['stride'])
                                 for L in self.layers[1:]]
      self.wt = [None] + [torch.empty(G, 3, 3, L['Cout'], L['Cin'], **f32) if self.needs_wt[l] else None
                          for l, L in enumerate(self.layers) if l >= 1]
      if self.split_top:
        L7 = self.layers[7]
        self.needs_wt7 = [ops.conv3x3_dgrad_needs_wt(L7['H'], L7['W'], L7['Cin'], d, L7['stride']) for d in self.dim_outs]
        self.wt[7] = [torch.empty(3, 3, d, L7['Cin'], **f32) if nw else None for d, nw in zip(self.dim_outs, self.needs_wt7)]
      if self.pad1:
        self.dw1p = torch.zeros(G, 3, 3, self.Cpad, self.layers[0]['Cout'], **f32)
      # one split-K workspace per layer: the slab sums that graph._ModelBase.backward_and_apply runs beside the fused bottom
      # read conv3..conv8's workspaces while conv2's filter gradient writes its own
      self.ws_l = [torch.empty(ops.conv3x3_wgrad_ws_bytes(G, Nf, L['H'], L['W'], L['Cin'], L['Cout'], L['stride']) // 4 + 4,
                               **f32) for L in self.layers]
      dsb = max(ops.conv3x3_dgrad_ws_bytes(G, Nf, L['H'], L['W'], L['Cin'], L['Cout'], L['stride'])
                for L in self.layers[1:])
      self.dws = torch.empty(dsb // 4 + 4, **f32)
      # Two streams, created here as when they carried the filter gradients of a multi-stream backward.  The optimiser's early
      # piece runs on the first beside the backward's bottom (graph._ModelBase.backward_and_apply); the second carries no work.  It
      # stays because the streams a process creates later (RCCL's, the data-parallel runner's) land on other hardware queues
      # without it: with one stream here 8 of the 11 forms of bench.py's dp_one_rank measured 3-12 us per step slower, beyond the
      # spread of four runs (profiles/one_path/README.md)
      self.sides = [torch.cuda.Stream(device=dev) for _ in range(2)] if dev.type == 'cuda' else []
      if self.fused_bottom:
        self.fws_fused = torch.empty(ops.conv2_dgrad_conv1_wgrad_ws_bytes(G) // 4 + 4, **f32)
    fsb = max(ops.conv3x3_fwd_ws_bytes(G, Nf, L['H'], L['W'], L['Cin'], L['Cout'], L['stride']) for L in self.layers)
    self.fws = torch.empty(fsb // 4 + 4, **f32)
    # The launch plan: which kernel runs each layer, decided here once (launch_fwd / launch_dgrad dispatch on it).  Forward: 'plain',
    # or the variant that also leaves the signs of its output for the backward -- conv1 one bit per value ('bits_rgb': straight from
    # the RGB variable, no padded kernel copy), conv2 16-bit fields, conv3 byte fields -- or conv8 per encoder.  Input gradient of
    # layer l (into dz[l-1]): 'plain', conv2's fused with conv1's filter gradient, conv3's from the 16-bit fields, conv4's LDS-staged
    # from the byte fields, conv8's per encoder.
    pick = lambda flag, variant: variant if flag else 'plain'
    top = pick(self.split_top, 'per_encoder')
    self.fwd_plan = [pick(self.relu_bits, 'bits' if self.pad1_copy or not self.pad1 else 'bits_rgb'), pick(self.relu_fields, 'fields16'),
                     pick(self.relu_fields3, 'fields8'), 'plain', 'plain', 'plain', 'plain', top]
    self.dgrad_plan = [None, pick(self.fused_bottom, 'fused_bottom'), pick(self.relu_fields, 'fields16'),
                       pick(self.relu_fields3, 'fields8'), 'plain', 'plain', 'plain', top]
    # conv7's input gradient and conv7's / conv8's filter gradients need only conv8's input gradient: one grid for the three
    self.top_one_grid = not self.split_top and self.layers[6]['stride'] == self.layers[7]['stride'] == 2

  def _w(self, l, g=0):
    return self.store.var('%s/conv%d/kernel' % (self.scopes[g], l + 1))

  def _b(self, l, g=0):
    return self.store.var('%s/conv%d/bias' % (self.scopes[g], l + 1))

  def _grad_view(self, l, g, kind):
    name = '%s/conv%d/%s' % (self.scopes[g], l + 1, kind)
    grad = self.store.grad(name)
    if self.late is None or l >= self.SPLIT:
      return grad
    staging, stride = self.late      # the same view, of encoder g's block of the staging buffer
    o = self.store.offsets[name] - self.store.offsets[self.scopes[g] + '/conv1/kernel'] + g * stride
    return staging[o:o + grad.numel()].view_as(grad)

  def _dw(self, l, g=0):
    return self._grad_view(l, g, 'kernel')

  def _db(self, l, g=0):
    return self._grad_view(l, g, 'bias')

  def _gs_g(self, l):
    """Group stride of layer l's gradient views (the arena's, or the late staging buffer's for conv1 / conv2)."""
    return self.late[1] if (self.late is not None and l < self.SPLIT) else self.gs_p

  def redirect_late_gradients(self, staging, late_ranges):
    """Data parallel (runtime.TrainStepRunner): the gradients of conv1 / conv2 -- the LATE bucket, written by the last
    launches of the backward -- go straight into ``staging`` (encoder g's block at g * len, same inner layout as the
    arena) instead of the gradient arena, so that the arena is not written while the early bucket is being reduced.
    Returns False if the late ranges are not the uniformly strided conv1 / conv2 blocks, or when called with
    ``staging=None``, which ends a redirection (the gradients go to the arena again)."""
    self.late = None
    if staging is None:
      return False
    off = self.store.offsets
    lo0 = off[self.scopes[0] + '/conv1/kernel']
    length = off[self.scopes[0] + '/conv%d/kernel' % (self.SPLIT + 1)] - lo0
    want = [(lo0 + g * self.gs_p, length) for g in range(self.G)]
    if [tuple(r) for r in late_ranges] != want or staging.numel() != self.G * length or not self.training:
      return False
    self.late = (staging, length)
    return True

  @property
  def features(self):
    """[G][Nf][h][w][dim_out] output of conv8 (endpoints['conv8'], graph.py:116)."""
    return self.acts[7]

  @property
  def dfeatures(self):
    return self.dz[7]

  def refresh_derived(self):
    """Re-derives the weight copies the kernels read (conv1's kernel padded to 4 input channels; the
    per-tap transposed kernels of the dgrad GEMMs).  Training calls it right after Adam (inside the
    Adam hipGraph), so the forward / backward graphs contain no pad or transpose launches."""
    G = self.G
    # only the layers whose input-gradient kernel reads the transposed copy (the LDS-staged ones read the HWIO kernel)
    ls = [l for l in range(1, 7 if self.split_top else 8) if self.needs_wt[l]]
    for g, needed in enumerate(self.needs_wt7):
      if needed:
        ops.derive_conv_weights([self._w(7, g)], [self.wt[7][g].unsqueeze(0)], [self.layers[7]['Cin']], [self.dim_outs[g]], 1, 0)
    pad = dict(pad_src=self._w(0), pad_dst=self.w1p, pad_cin=self.Cin, pad_cin_padded=self.Cpad,
               pad_cout=self.layers[0]['Cout']) if self.pad1_copy else {}
    if ls or pad:
      ops.derive_conv_weights([self._w(l) for l in ls], [self.wt[l] for l in ls], [self.layers[l]['Cin'] for l in ls],
                              [self.layers[l]['Cout'] for l in ls], G, self.gs_p, **pad)
    self.derived_version = self.store.version

  # -- single launches (also timed one by one by bench.py's per-layer table) ---------------------------
  # One helper per direction gives layer l's arguments as (tensors, (groups, group strides ...), (N, H, W, Cin, Cout, stride)).
  # ``g``: encoder g alone -- conv8 under split_top, whose outputs, gradients and kernel copies are one tensor per encoder: buf[g] is
  # encoder g's part of a grouped buffer and of such a list alike, and a single group has no strides.

  def _shape(self, l, g=None):
    L = self.layers[l]
    return (self.Nf, L['H'], L['W'], L['Cin'], L['Cout'] if g is None else self.dim_outs[g], L['stride'])

  def _fwd_operands(self, l, g=None):
    """(y, x, w, b), (G, gs_x, gs_w, gs_b, gs_y), shape."""
    x, y = self.x_in if l == 0 else self.acts[l - 1], self.acts[l]
    if g is not None:
      return (y[g], x[g], self._w(l, g), self._b(l, g)), (1, 0, 0, 0, 0), self._shape(l, g)
    w, gs_w = (self.w1p, self.w1p[0].numel()) if (l == 0 and self.pad1_copy) else (self._w(l), self.gs_p)
    return (y, x, w, self._b(l)), (self.G, x[0].numel(), gs_w, self.gs_p, y[0].numel()), self._shape(l)

  def _dgrad_operands(self, l, g=None):
    """(dx, dz, wt, x, w), (G, gs_dz, gs_wt, gs_dx, gs_w), shape; x = the layer's input, whose sign is the ReluGrad mask."""
    dx, dz, wt, x = self.dz[l - 1], self.dz[l], self.wt[l], self.acts[l - 1]
    if g is not None:
      return (dx[g], dz[g], wt[g], x[g], self._w(l, g)), (1, 0, 0, 0, 0), self._shape(l, g)
    return ((dx, dz, wt, x, self._w(l)), (self.G, dz[0].numel(), wt[0].numel() if wt is not None else 0, dx[0].numel(), self.gs_p),
            self._shape(l))

  def _wgrad_operands(self, l, g=None):
    """(dw, db, x, dz), (G, gs_x, gs_dz, gs_dw, gs_db), shape; conv1's filter gradient in the channel-padded layout where that exists."""
    x, dz = self.x_in if l == 0 else self.acts[l - 1], self.dz[l]
    if g is not None:
      return (self._dw(l, g), self._db(l, g), x[g], dz[g]), (1, 0, 0, 0, 0), self._shape(l, g)
    dw, gs_dw = (self.dw1p, self.dw1p[0].numel()) if (l == 0 and self.pad1) else (self._dw(l), self._gs_g(l))
    return (dw, self._db(l), x, dz), (self.G, x[0].numel(), dz[0].numel(), gs_dw, self._gs_g(l)), self._shape(l)

  def launch_fwd(self, l):
    plan = self.fwd_plan[l]
    if plan in ('plain', 'per_encoder'):
      for g in range(self.G) if plan == 'per_encoder' else (None,):
        tensors, groups, shape = self._fwd_operands(l, g)
        ops.conv3x3_fwd_into(*tensors, *groups, *shape, relu=True, ws=self.fws)
      return
    fwd = {'bits': ops.conv1_fwd_relu_bits_into, 'bits_rgb': ops.conv1_fwd_relu_bits_rgb_into,
           'fields16': ops.conv2_fwd_relu_fields_into, 'fields8': ops.conv3_fwd_relu_fields_into}[plan]
    (y, x, w, b), groups, shape = self._fwd_operands(l)
    signs = (self.bits1, self.fields2, self.fields3)[l]
    fwd(y, signs, x, w, b, *groups, signs[0].numel(), *shape[:3])

  def launch_wgrad(self, l, pending=None):
    """Filter + bias gradient of layer l (skipped for conv1 when the encoder bottom is fused: launch_dgrad(1) does it).
    ``pending`` (a list): the kernel's final slab sum is deferred to ``ops.slab_reduce_batch(pending)``."""
    if l == 0 and self.fused_bottom:
      return
    if l == 7 and self.split_top:
      for g in range(self.G):
        tensors, groups, shape = self._wgrad_operands(l, g)
        ops.conv3x3_wgrad_into(*tensors, *groups, *shape, self.ws_l[l])
      return
    repack = l == 0 and self.pad1     # the padded gradient is repacked right below: its slab sum is not deferred
    tensors, groups, shape = self._wgrad_operands(l)
    ops.conv3x3_wgrad_into(*tensors, *groups, *shape, self.ws_l[l], pending=None if repack else pending,
                           reserved_cus=self.reserved_cus if (l == 1 and pending is not None) else 0)
    if repack:
      for g in range(self.G):
        ops.pad_mid_into(self._dw(0, g), self.dw1p[g], 9, self.Cpad, self.Cin, shape[4])

  def _wgrad_args(self, l):
    (dw, db, x, dz), (_, gs_x, gs_dz, gs_dw, gs_db), (N, H, W, Cin, Cout, _) = self._wgrad_operands(l)
    return dict(dw=dw, db=db, x=x, dz=dz, gs_x=gs_x, gs_dz=gs_dz, gs_dw=gs_dw, gs_db=gs_db, N=N, H=H, W=W, Cin=Cin, Cout=Cout,
                ws=self.ws_l[l])

  def launch_wgrad_top_pair(self, pending=None):
    """conv7's and conv8's filter gradients as ONE launch (both are ready once conv8's input gradient exists; each alone is
    432 blocks on 256 CUs): False when the shapes are outside the paired kernel (the caller launches them one by one)."""
    return ops.conv3x3_wgrad_pair_into(self._wgrad_args(6), self._wgrad_args(7), self.G, self.layers[6]['stride'], pending=pending)

  def launch_top_bwd(self, l, wgrads, pending=None):
    """Layer l's input gradient AND the filter gradients of layers ``wgrads`` as one heterogeneous launch (independent work
    that needs only dz[l]): l = 6 with (6, 7)."""
    (dx, dz, wt, x, w), (G, gs_dz, gs_wt, gs_dx, gs_w), (N, H, W, Cin, Cout, stride) = self._dgrad_operands(l)
    d = dict(dx=dx, dz=dz, wt=wt, ymask=x, w=w, gs_dz=gs_dz, gs_w=gs_w, gs_wt=gs_wt, gs_dx=gs_dx, N=N, H=H, W=W, Cin=Cin, Cout=Cout,
             ws=self.dws)
    return ops.conv_top_bwd_into(d, self._wgrad_args(wgrads[0]), self._wgrad_args(wgrads[1]) if len(wgrads) > 1 else None, G,
                                 stride, pending=pending)

  def launch_dgrad(self, l, pending=None):
    """Input gradient of layer l >= 1 into dz[l-1] (ReluGrad of the layer below fused).  With the fused encoder
    bottom, l == 1 also produces conv1's filter / bias gradient: dz1 has no other consumer and stays on chip
    (805 MB less written and read again per step, one big launch less)."""
    plan = self.dgrad_plan[l]
    if plan == 'fused_bottom':
      # the kernel writes conv1's gradient in the variable's own [3][3][Cin][32] layout (no padded copy to repack) and reads
      # the sign bits of conv1's output (relu_bits) for its ReluGrad
      dz, (N, H, W, _, _, _) = self.dz[l], self._shape(l)
      ops.conv2_dgrad_conv1_wgrad_bits_into(self._dw(0), self._db(0), dz, self._w(1), self.bits1, self.x_in, self.G,
                                            dz[0].numel(), self.gs_p, self.bits1[0].numel(), self.x_in[0].numel(),
                                            self._gs_g(0), self._gs_g(0), N, H, W, self.fws_fused,
                                            real_channels=self.Cin, pending=pending, reserved_cus=self.reserved_cus)
      return
    for g in range(self.G) if plan == 'per_encoder' else (None,):
      (dx, dz, wt, x, w), (G, gs_dz, gs_wt, gs_dx, gs_w), shape = self._dgrad_operands(l, g)
      if plan in ('plain', 'per_encoder'):
        ops.conv3x3_dgrad_into(dx, dz, wt, x, G, gs_dz, gs_wt, gs_dx, *shape, ws=self.dws, w=w, gs_w=gs_w)
      elif plan == 'fields8':
        ops.conv3x3_dgrad_relu_fields_into(dx, dz, w, self.fields3, G, gs_dz, gs_w, self.fields3[0].numel(), gs_dx, *shape)
      else:
        ops.conv3_dgrad_relu_fields_into(dx, dz, w, self.fields2, G, gs_dz, gs_w, self.fields2[0].numel(), gs_dx, *shape[:3],
                                         reserved_cus=self.reserved_cus)

  def forward(self, state=None):
    """``state`` (one-step decoders): dict(state, state_stride, feat_off, Ctot, jnt, jnt_stride, jnt_off, J) of the state
    concat that consumes the features; it then rides in the epilogue of the top layer's split-K sum where that exists.
    Returns True if it did (else the caller launches the concat)."""
    if not self.lazy_refresh or self.derived_version != self.store.version:
      self.refresh_derived()
    top = len(self.layers) - 1
    for l in range(top):
      self.launch_fwd(l)
    # the state concat of a one-step decoder rides in conv8's split-K epilogue
    if state is not None and not self.split_top:
      tensors, groups, shape = self._fwd_operands(top)
      if ops.conv3x3_fwd_state_into(*tensors, *groups, *shape, self.fws, **state):
        return True
    self.launch_fwd(top)
    return False

  # -- the backward in two halves: every launch appends its deferred slab sum to ``pending``, graph._ModelBase.backward launches them

  def backward_upper(self, pending):
    """Expects ``self.dz[7]`` = d(loss)/d(pre-activation of conv8) (ReluGrad already applied).  conv8 .. conv(SPLIT+1), the last
    one's input gradient left to ``backward_bottom``."""
    first = 7
    if self.top_one_grid:
      self.launch_dgrad(7, pending)
      if not self.launch_top_bwd(6, (6, 7), pending):
        if not self.launch_wgrad_top_pair(pending):
          self.launch_wgrad(7, pending)
          self.launch_wgrad(6, pending)
        self.launch_dgrad(6, pending)
      first = 5
    for l in range(first, self.SPLIT, -1):
      self.launch_wgrad(l, pending)
      self.launch_dgrad(l, pending)
    self.launch_wgrad(self.SPLIT, pending)

  def backward_bottom(self, pending, before_bottom=None):
    """conv(SPLIT+1)'s input gradient, then conv(SPLIT) .. conv1 (whose input is data: no input gradient).  ``before_bottom(pending)``
    is called right in front of the LAST big launch of the chain, conv2's input gradient (+ conv1's filter gradient when the bottom
    is fused) -- graph.BesideBottom releases side work there."""
    self.launch_dgrad(self.SPLIT, pending)
    for l in range(self.SPLIT - 1, 0, -1):
      self.launch_wgrad(l, pending)
      if l == 1 and before_bottom is not None:
        before_bottom(pending)
      self.launch_dgrad(l, pending)
    self.launch_wgrad(0, pending)

  # -- beyond the training backward: the gradient of conv1's INPUT, for saliency maps ----------------------

  def check_input_gradient(self):
    """ValueError unless ``input_gradient`` can run on this stack."""
    if not self.training:
      raise ValueError('input gradients need a training stack (an inference stack keeps no gradient buffers)')
    L0 = self.layers[0]
    if self.Cpad != 4 or self.Cin not in (3, 4) or L0['Cout'] != 32 or L0['stride'] != 1:
      raise ValueError('input gradients: geeco_conv1_dgrad serves conv1 of the reference encoder (3 or 4 -> 32 channels, stride 1), '
                       'not %d -> %d stride %d' % (self.Cin, L0['Cout'], L0['stride']))

  def input_gradient(self, chunk_frames=96):
    """d(loss)/d(``x_in``) into ``dx_in`` (shaped like ``x_in``; channel 3 of an RGB stack is 0), which it returns.  Valid after
    ``backward_upper`` has left ``dz[1]``; the training backward, its launches and its buffers stay as they are.  Per encoder and per
    chunk of at most ``chunk_frames`` frames: conv2's input gradient under conv1's ReLU decisions (``geeco_conv3x3_dgrad``, the generic
    entry: every shape) into a chunk buffer, then ``geeco_conv1_dgrad``.  The chunk bounds the workspace: conv1's pre-activation
    gradient is 8.4 MB per 256 x 256 frame (805 MB at 96 frames, 8.6 GB for the 1024 frames of a K = 32 batch of 32)."""
    self.check_input_gradient()
    chunk = max(1, min(int(chunk_frames), self.Nf))
    L0, L1 = self.layers[0], self.layers[1]
    H, W = L0['H'], L0['W']
    if getattr(self, 'dx_in', None) is None:
      self.dx_in = torch.zeros_like(self.x_in)
    if getattr(self, 'dz1_chunk', None) is None or self.dz1_chunk.shape[0] < chunk:
      self.dz1_chunk = torch.empty(chunk, H, W, L0['Cout'], dtype=torch.float32, device=self.x_in.device)
    for g in range(self.G):
      wt = self.wt[1][g] if self.wt[1] is not None else None
      for f0 in range(0, self.Nf, chunk):
        n = min(chunk, self.Nf - f0)
        ops.conv3x3_dgrad_into(self.dz1_chunk, self.dz[1][g][f0:f0 + n], wt, self.acts[0][g][f0:f0 + n], 1, 0, 0, 0, n, L1['H'], L1['W'],
                               L1['Cin'], L1['Cout'], L1['stride'], ws=self.dws, w=self._w(1, g), gs_w=0)
        if not ops.conv1_dgrad_into(self.dx_in[g][f0:f0 + n], self.dz1_chunk, self._w(0, g), 1, 0, 0, 0, n, H, W, self.Cin, L0['Cout']):
          raise RuntimeError('geeco_conv1_dgrad does not serve this conv1')      # (check_input_gradient said it would)
    return self.dx_in
