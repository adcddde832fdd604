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

  def __init__(self, store: VariableStore, scopes, Nf, H, W, Cin, dim_out, training):
    """``dim_out``: conv8's output channels, one int or one per encoder (dim_s_obs / dim_s_dyn / dim_s_diff,
    graph.py:390,394,402).  With unequal values conv1..conv7 still run as grouped launches and conv8 (the only layer
    whose shape differs) runs once per encoder (``split_top``)."""
    self.store, self.scopes, self.G, self.Nf = store, list(scopes), len(scopes), Nf
    self.H, self.W, self.Cin = H, W, Cin
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
      self.gs_p = gs
    else:
      self.gs_p = 0
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
      self.ws = self.ws_l[0]
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

  def _w(self, l, g=0):
    return self.store.var('%s/conv%d/kernel' % (self.scopes[g], l + 1))

  def _b(self, l, g=0):
    return self.store.var('%s/conv%d/bias' % (self.scopes[g], l + 1))

  def _grad_view(self, l, g, kind):
    name = '%s/conv%d/%s' % (self.scopes[g], l + 1, kind)
    if self.late is None or l >= ConvEncoderStack.SPLIT:
      return self.store.grad(name)
    staging, stride = self.late
    shp = self.store.shapes[name]
    o = self.store.offsets[name] - self.store.offsets[self.scopes[g] + '/conv1/kernel'] + g * stride
    n = 1
    for d in shp:
      n *= int(d)
    return staging[o:o + n].view(*shp)

  def _dw(self, l, g=0):
    return self._grad_view(l, g, 'kernel')

  def _db(self, l, g=0):
    return self._grad_view(l, g, 'bias')

  def _gs_g(self, l):
    """Group stride of layer l's gradient views (the arena's, or the late staging buffer's for conv1 / conv2)."""
    return self.late[1] if (self.late is not None and l < ConvEncoderStack.SPLIT) else self.gs_p

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
    length = off[self.scopes[0] + '/conv%d/kernel' % (ConvEncoderStack.SPLIT + 1)] - lo0
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
    ls = [l for l in range(1, 7 if self.split_top else 8) if self.needs_wt[l]] if self.training else []
    if self.training and self.split_top:
      L7 = self.layers[7]
      for g in range(G):
        if self.wt[7][g] is not None:
          ops.derive_conv_weights([self._w(7, g)], [self.wt[7][g].unsqueeze(0)], [L7['Cin']], [self.dim_outs[g]], 1, 0)
    pad = dict(pad_src=self._w(0), pad_dst=self.w1p, pad_cin=self.Cin, pad_cin_padded=self.Cpad,
               pad_cout=self.layers[0]['Cout']) if self.pad1_copy else {}
    if ls or pad:
      ops.derive_conv_weights([self._w(l) for l in ls], [self.wt[l] for l in ls], [self.layers[l]['Cin'] for l in ls],
                              [self.layers[l]['Cout'] for l in ls], G, self.gs_p, **pad)
    self.derived_version = self.store.version

  # -- single launches (also timed one by one by bench.py's per-layer table) ---------------------------

  def launch_fwd(self, l):
    G, Nf, L = self.G, self.Nf, self.layers[l]
    if l == 7 and self.split_top:
      for g in range(G):
        ops.conv3x3_fwd_into(self.acts[7][g], self.acts[6][g], self._w(7, g), self._b(7, g), 1, 0, 0, 0, 0, Nf, L['H'], L['W'],
                             L['Cin'], self.dim_outs[g], L['stride'], relu=True, ws=self.fws)
      return
    x = self.x_in if l == 0 else self.acts[l - 1]
    y = self.acts[l]
    if l == 0 and self.pad1:
      w, gs_w = self.w1p, self.w1p[0].numel()
    else:
      w, gs_w = self._w(l), self.gs_p
    if l == 2 and self.training and self.relu_fields3:
      ops.conv3_fwd_relu_fields_into(y, self.fields3, x, w, self._b(2), G, x[0].numel(), gs_w, self.gs_p, y[0].numel(),
                                     self.fields3[0].numel(), Nf, L['H'], L['W'])
      return
    if l == 1 and self.training and self.relu_fields:
      ops.conv2_fwd_relu_fields_into(y, self.fields2, x, w, self._b(1), G, x[0].numel(), gs_w, self.gs_p, y[0].numel(),
                                     self.fields2[0].numel(), Nf, L['H'], L['W'])
      return
    if l == 0 and self.training and self.relu_bits and self.pad1 and not self.pad1_copy:
      ops.conv1_fwd_relu_bits_rgb_into(y, self.bits1, x, self._w(0), self._b(0), G, x[0].numel(), self.gs_p, self.gs_p, y[0].numel(),
                                       self.bits1[0].numel(), Nf, L['H'], L['W'])
      return
    if l == 0 and self.training and self.relu_bits:
      ops.conv1_fwd_relu_bits_into(y, self.bits1, x, w, self._b(0), G, x[0].numel(), gs_w, self.gs_p, y[0].numel(),
                                   self.bits1[0].numel(), Nf, L['H'], L['W'])
      return
    ops.conv3x3_fwd_into(y, x, w, self._b(l), G, x[0].numel(), gs_w, self.gs_p, y[0].numel(), Nf, L['H'], L['W'],
                         L['Cin'], L['Cout'], L['stride'], relu=True, ws=self.fws)

  def launch_wgrad(self, l, pending=None):
    """Filter + bias gradient of layer l (skipped for conv1 when the encoder bottom is fused: launch_dgrad(1) does it).
    ``pending`` (a list): the kernel's final slab sum is deferred to ``ops.slab_reduce_batch(pending)``."""
    G, Nf, L = self.G, self.Nf, self.layers[l]
    if l == 0 and self.fused_bottom:
      return
    if l == 7 and self.split_top:
      for g in range(G):
        ops.conv3x3_wgrad_into(self._dw(7, g), self._db(7, g), self.acts[6][g], self.dz[7][g], 1, 0, 0, 0, 0, Nf, L['H'],
                               L['W'], L['Cin'], self.dim_outs[g], L['stride'], self.ws_l[7])
      return
    x = self.x_in if l == 0 else self.acts[l - 1]
    dz = self.dz[l]
    if l == 0 and self.pad1:
      dw, gs_dw = self.dw1p, self.dw1p[0].numel()
    else:
      dw, gs_dw = self._dw(l), self._gs_g(l)
    if l == 0 and self.pad1:
      pending = None     # the padded gradient is repacked right below
    ops.conv3x3_wgrad_into(dw, self._db(l), x, dz, G, x[0].numel(), dz[0].numel(), gs_dw, self._gs_g(l), Nf, L['H'],
                           L['W'], L['Cin'], L['Cout'], L['stride'], self.ws_l[l], pending=pending,
                           reserved_cus=self.reserved_cus if (l == 1 and pending is not None) else 0)
    if l == 0 and self.pad1:
      for g in range(G):
        ops.pad_mid_into(self._dw(0, g), self.dw1p[g], 9, self.Cpad, self.Cin, L['Cout'])

  def _wgrad_args(self, l):
    L = self.layers[l]
    x, dz = self.acts[l - 1], self.dz[l]
    return dict(dw=self._dw(l), db=self._db(l), x=x, dz=dz, gs_x=x[0].numel(), gs_dz=dz[0].numel(), gs_dw=self._gs_g(l),
                gs_db=self._gs_g(l), N=self.Nf, H=L['H'], W=L['W'], Cin=L['Cin'], Cout=L['Cout'], ws=self.ws_l[l])

  def launch_wgrad_top_pair(self, pending=None):
    """conv7's and conv8's filter gradients as ONE launch (both are ready once conv8's input gradient exists; each alone is
    432 blocks on 256 CUs): False when the shapes are outside the paired kernel (the caller launches them one by one)."""
    return ops.conv3x3_wgrad_pair_into(self._wgrad_args(6), self._wgrad_args(7), self.G, self.layers[6]['stride'], pending=pending)

  def launch_top_bwd(self, l, wgrads, pending=None):
    """Layer l's input gradient AND the filter gradients of layers ``wgrads`` as one heterogeneous launch (independent work
    that needs only dz[l]): l = 6 with (6, 7)."""
    L = self.layers[l]
    wt = self.wt[l]
    d = dict(dx=self.dz[l - 1], dz=self.dz[l], wt=wt, ymask=self.acts[l - 1], w=self._w(l), gs_dz=self.dz[l][0].numel(),
             gs_w=self.gs_p, gs_wt=wt[0].numel() if wt is not None else 0, gs_dx=self.dz[l - 1][0].numel(), N=self.Nf, H=L['H'],
             W=L['W'], Cin=L['Cin'], Cout=L['Cout'], ws=self.dws)
    return ops.conv_top_bwd_into(d, self._wgrad_args(wgrads[0]), self._wgrad_args(wgrads[1]) if len(wgrads) > 1 else None, self.G,
                                 L['stride'], pending=pending)

  def launch_dgrad(self, l, pending=None):
    """Input gradient of layer l >= 1 into dz[l-1] (ReluGrad of the layer below fused).  With the fused encoder
    bottom, l == 1 also produces conv1's filter / bias gradient: dz1 has no other consumer and stays on chip
    (805 MB less written and read again per step, one big launch less)."""
    G, Nf, L = self.G, self.Nf, self.layers[l]
    if l == 7 and self.split_top:
      for g in range(G):
        ops.conv3x3_dgrad_into(self.dz[6][g], self.dz[7][g], self.wt[7][g], self.acts[6][g], 1, 0, 0, 0, Nf, L['H'], L['W'],
                               L['Cin'], self.dim_outs[g], L['stride'], ws=self.dws, w=self._w(7, g), gs_w=0)
      return
    x = self.acts[l - 1]
    dz = self.dz[l]
    if l == 1 and self.fused_bottom:
      # the kernel writes conv1's gradient in the variable's own [3][3][Cin][32] layout (no padded copy to repack) and reads
      # the sign bits of conv1's output (relu_bits) for its ReluGrad
      ops.conv2_dgrad_conv1_wgrad_bits_into(self._dw(0), self._db(0), dz, self._w(1), self.bits1, self.x_in, G,
                                            dz[0].numel(), self.gs_p, self.bits1[0].numel(), self.x_in[0].numel(),
                                            self._gs_g(0), self._gs_g(0), Nf, L['H'], L['W'], self.fws_fused,
                                            real_channels=self.Cin, pending=pending, reserved_cus=self.reserved_cus)
      return
    wt = self.wt[l]
    dx = self.dz[l - 1]
    if l == 3 and self.relu_fields3:
      ops.conv3x3_dgrad_relu_fields_into(dx, dz, self._w(3), self.fields3, G, dz[0].numel(), self.gs_p, self.fields3[0].numel(),
                                         dx[0].numel(), Nf, L['H'], L['W'], L['Cin'], L['Cout'], L['stride'])
      return
    if l == 2 and self.relu_fields:
      ops.conv3_dgrad_relu_fields_into(dx, dz, self._w(2), self.fields2, G, dz[0].numel(), self.gs_p, self.fields2[0].numel(),
                                       dx[0].numel(), Nf, L['H'], L['W'], reserved_cus=self.reserved_cus)
      return
    ops.conv3x3_dgrad_into(dx, dz, wt, x, G, dz[0].numel(), wt[0].numel() if wt is not None else 0, dx[0].numel(), Nf, L['H'],
                           L['W'], L['Cin'], L['Cout'], L['stride'], ws=self.dws, w=self._w(l), gs_w=self.gs_p)

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
      G, Nf, L = self.G, self.Nf, self.layers[top]
      x, y = self.acts[top - 1], self.acts[top]
      if ops.conv3x3_fwd_state_into(y, x, self._w(top), self._b(top), G, x[0].numel(), self.gs_p, self.gs_p, y[0].numel(), Nf,
                                    L['H'], L['W'], L['Cin'], L['Cout'], L['stride'], self.fws, **state):
        return True
    self.launch_fwd(top)
    return False

  def backward(self, hi=7, lo=0, prepare=None, defer_dgrad=False, lead_dgrad=None, defer_sums=None, before_bottom=None):
    """Expects ``self.dz[7]`` = d(loss)/d(pre-activation of conv8) (ReluGrad already applied).  Runs layers
    hi..lo (the data-parallel runner splits the chain at conv3 / conv2 to start the gradient exchange early).
    ``prepare`` = (global_step, lr, scal): the optimiser's per-step scalars ride in this part's slab-sum launch.
    ``defer_dgrad``: layer lo's INPUT gradient is left to the next part, which opens with it (``lead_dgrad=lo``): every
    gradient of the early bucket exists once layer lo's filter gradient does, so the bucket leaves a launch earlier.
    ``defer_sums`` (a list): this part's pending slab sums are handed to the caller instead of launched (``prepare`` must be None).
    ``before_bottom``: called right before the LAST launch of the chain, conv2's input gradient (+ conv1's filter gradient when
    the bottom is fused) -- graph._ModelBase.backward_and_apply releases the optimiser's early piece onto a second stream there."""
    assert defer_sums is None or prepare is None
    pending = []   # slab sums of all layers of this part: one launch at the end
    # conv7's input gradient and conv7's / conv8's filter gradients need only conv8's input gradient: one grid for the three
    pair_top = (hi == 7 and lo <= 6 and not self.split_top
                and self.layers[6]['stride'] == self.layers[7]['stride'] == 2)
    if lead_dgrad is not None:
      self.launch_dgrad(lead_dgrad, pending)
    for l in range(hi, lo - 1, -1):
      if pair_top and l == 7:
        self.launch_dgrad(7, pending)
        continue
      if pair_top and l == 6:
        if self.launch_top_bwd(6, (6, 7), pending):
          continue
        if not self.launch_wgrad_top_pair(pending):
          self.launch_wgrad(7, pending)
          self.launch_wgrad(6, pending)
        self.launch_dgrad(6, pending)
        continue
      self.launch_wgrad(l, pending)
      if l == 0 or (l == lo and defer_dgrad):
        break   # conv1's input is data: no dgrad / the next part opens with this layer's
      if l == 1 and before_bottom is not None:
        before_bottom(pending)
      self.launch_dgrad(l, pending)
      if l == 1 and self.fused_bottom:
        break
    if defer_sums is not None:
      defer_sums.extend(pending)
      return
    if pending or prepare is not None:
      ops.slab_reduce_batch(pending, prepare)

  # backward(part='upper') = layers 7..SPLIT, 'bottom' = SPLIT-1..0, which opens with layer SPLIT's INPUT gradient (round 4 cut after it)
  SPLIT = 2
