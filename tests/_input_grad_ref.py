"""float64 restatements of the input-gradient kernels (include/geeco_hip.h: geeco_conv1_dgrad, geeco_pack_pixels_bwd,
geeco_dynimg_bwd), shared by tests/test_input_grad_cpu.py and tests/test_input_grad_gpu.py; and, below them, the launch-variant
table of tests/test_input_grad_variants_gpu.py: CASES (one record per launch form of the three entry points), the host side of
each launch (layouts, the vector width V, block and tile counts, the workspace), seeded inputs with planted extrema and ties,
per-element rounding bounds derived from the kernels' operation order, and ``input_grad_compare``.
tests/test_input_grad_cover_cpu.py shows on the host that the table holds every edge and that the comparison rejects wrong kernels."""
import numpy as np
import torch

import _primitive_refs as P
from oracle import geeco_oracle as O


def conv1_dgrad_ref(dz1, w1):
  """dx[f][y][x][ci] = sum_{ky,kx,co} dz1[f][y+1-ky][x+1-kx][co] w1[ky][kx][ci][co]: dz1 [F][H][W][Co], w1 [3][3][Cin][Co] ->
  [F][H][W][Cin], float64 (explicit shifted sums; no autograd)."""
  dz1, w1 = np.asarray(dz1, np.float64), np.asarray(w1, np.float64)
  F, H, W, _ = dz1.shape
  pad = np.zeros((F, H + 2, W + 2, dz1.shape[3]))
  pad[:, 1:H + 1, 1:W + 1] = dz1
  dx = np.zeros((F, H, W, w1.shape[2]))
  for ky in range(3):
    for kx in range(3):
      # dz1[y + 1 - ky][x + 1 - kx] = pad[y + 2 - ky][x + 2 - kx]
      dx += np.einsum('fyxo,io->fyxi', pad[:, 2 - ky:2 - ky + H, 2 - kx:2 - kx + W], w1[ky, kx])
  return dx


def pack_bwd_ref(d_dst, C1, d_src=None, C2=0, d_src2=None):
  """The adjoint of geeco_pack_pixels in the arrays' own dtype: d_dst [..., Cpad] -> (d_src [..., C1], d_src2 [..., C2] or None);
  ``d_src`` / ``d_src2`` given: added to (one addition per element)."""
  d_dst = np.asarray(d_dst)
  a = d_dst[..., :C1] if d_src is None else np.asarray(d_src) + d_dst[..., :C1]
  b = None
  if C2:
    b = d_dst[..., C1:C1 + C2] if d_src2 is None else np.asarray(d_src2) + d_dst[..., C1:C1 + C2]
  return a, b


def dynimg_bwd_ref(g, frames, alpha=None):
  """The adjoint of the normalised dynamic image, float64, TF 1.15's tie rule (reduce_min / reduce_max share their gradient evenly
  among equal extrema): g [N][...] (gradient of out), frames [N][K][...] -> d_frames [N][K][...].
    D = sum_t alpha_t X_t, r = max - min + 1e-6, out = (D - min) / r,
    dD_i = g_i / r + [D_i == min] (sum_j g_j (out_j - 1) / r) / n_min - [D_i == max] (sum_j g_j out_j / r) / n_max."""
  g, frames = np.asarray(g, np.float64), np.asarray(frames, np.float64)
  N, K = frames.shape[:2]
  alpha = np.asarray(O.dynimg_alpha(K) if alpha is None else alpha, np.float64)
  out = np.zeros_like(frames)
  for n in range(N):
    D = np.tensordot(alpha, frames[n], axes=(0, 0))
    mn, mx = D.min(), D.max()
    r = mx - mn + 1e-6
    o = (D - mn) / r
    is_min, is_max = D == mn, D == mx
    dD = g[n] / r + is_min * ((g[n] * (o - 1.0)).sum() / r) / is_min.sum() - is_max * ((g[n] * o).sum() / r) / is_max.sum()
    out[n] = alpha.reshape((K,) + (1,) * D.ndim) * dD
  return out


def dynimg_autograd(g, frames):
  """The same through autograd of the oracle's ``dynimg`` (float64): equal to ``dynimg_bwd_ref`` wherever no two elements tie for
  an extremum -- torch's ``min(dim)`` sends the whole term to ONE index."""
  x = torch.tensor(np.asarray(frames, np.float64), requires_grad=True)
  O.dynimg(x).backward(torch.tensor(np.asarray(g, np.float64)))
  return x.grad.numpy()


def plant_extrema(frames, seed=0, margin=0.25):
  """In place: per sample one pixel value raised in every frame with a positive coefficient (and lowered where it is negative), one
  the other way round, so that the sample's D has a unique maximum and minimum with a wide margin (inputs in [0, 1])."""
  N, K = frames.shape[:2]
  alpha = O.dynimg_alpha(K).astype(np.float64)
  r = np.random.default_rng(seed)
  flat = frames.reshape(N, K, -1)
  for n in range(N):
    i, j = r.choice(flat.shape[2], 2, replace=False)
    for t in range(K):
      up = alpha[t] > 0
      flat[n, t, i] = 1.0 + margin if up else -margin
      flat[n, t, j] = -margin if up else 1.0 + margin
  return frames


def extrema_margin(frames):
  """min over samples of (D_max - second largest, second smallest - D_min), float64."""
  frames = np.asarray(frames, np.float64)
  N, K = frames.shape[:2]
  alpha = O.dynimg_alpha(K).astype(np.float64)
  worst = np.inf
  for n in range(N):
    D = np.sort(np.tensordot(alpha, frames[n], axes=(0, 0)).reshape(-1))
    worst = min(worst, D[-1] - D[-2], D[1] - D[0])
  return float(worst)


# ==========================================================================================================================
# The launch variants (tests/test_input_grad_variants_gpu.py, tests/test_input_grad_cover_cpu.py)
# ==========================================================================================================================
U = P.U                          # unit roundoff of float32, 2^-24
DIV_U = P.DIV_U                  # a float division, in units of U (_primitive_refs: correctly rounded or not, under 2.5 ulp)
SECOND = 1.0 + 2.0 ** -10        # the products of two relative errors, each far below 2^-10 here, on top of a first-order sum
F32 = np.float32
HI, LO = 1.25, -0.25             # planted pixel values (plant_extrema's): outside the [0, 1) of every other pixel
C1D_TY, C1D_TX, C1D_CO = 8, 32, 32      # geeco_conv1_dgrad's tile and channel count
DYN_MAXK = 64
MARGIN = 1e-3                    # between an extremum of D and the next distinct value, float64: fp32 and fp64 agree on positions


def gamma(k):
  """k roundings in a row: (1 + U)^k - 1 <= k U / (1 - k U)."""
  return k * U / (1.0 - k * U)


def cdiv(a, b):
  return -(-a // b)


class Case:
  def __init__(self, index, entry, id, **kw):
    self.__dict__.update(kw, index=index, entry=entry, id='%s-%s' % (entry, id))

  def __repr__(self):
    return self.id

  def replace(self, **kw):
    d = dict(self.__dict__)
    d.update(kw)
    c = Case.__new__(Case)
    c.__dict__.update(d)
    return c


def _build():
  cases = []

  def add(entry, id, **kw):
    cases.append(Case(len(cases), entry, id, **kw))

  # ---- geeco_conv1_dgrad: every (H, W) around the 8 x 32 tile with both Cin; the four group forms and F in {1, 2} in rotation
  forms = ('g1', 'dense', 'padded', 'shared_w')
  i = 0
  for Cin in (3, 4):
    for H, W in ((1, 1), (8, 32), (9, 33), (7, 31), (16, 64), (17, 65)):
      form, F = forms[i % 4], 1 + (i // 2) % 2
      add('conv1', '%dx%d-cin%d-F%d-%s' % (H, W, Cin, F, form), H=H, W=W, Cin=Cin, F=F, form=form, exact=False)
      i += 1
  add('conv1', '9x33-cin3-F2-dense-int', H=9, W=33, Cin=3, F=2, form='dense', exact=True)
  add('conv1', '17x65-cin4-F1-padded-int', H=17, W=65, Cin=4, F=1, form='padded', exact=True)

  # ---- geeco_pack_pixels_bwd: K > 1 = sample views of an [N][K] stack (frame t), as graph.py passes them
  def pk(id, C1, C2, Cpad, HW, form, acc, K=1, N=2):
    add('pack', id, C1=C1, C2=C2, Cpad=Cpad, HW=HW, form=form, acc=acc, K=K, t=K // 2, N=N)
  pk('c3+0-pad4-hw255-src-strided', 3, 0, 4, 255, 'src', (0, 0), K=3)
  pk('c3+1-pad4-hw256-both-acc00-strided', 3, 1, 4, 256, 'both', (0, 0), K=4, N=3)
  pk('c3+1-pad4-hw257-both-acc10', 3, 1, 4, 257, 'both', (1, 0))
  pk('c3+1-pad4-hw1-both-acc01', 3, 1, 4, 1, 'both', (0, 1))
  pk('c3+1-pad4-hw255-both-acc11-strided', 3, 1, 4, 255, 'both', (1, 1), K=2)
  pk('c4+0-pad4-hw257-src-acc', 4, 0, 4, 257, 'src', (1, 0))
  pk('c3+1-pad8-hw256-both-acc01', 3, 1, 8, 256, 'both', (0, 1))
  pk('c1+2-pad3-hw257-both-acc10-strided', 1, 2, 3, 257, 'both', (1, 0), K=3)
  pk('c3+1-pad4-hw255-src2-only-acc', 3, 1, 4, 255, 'src2', (0, 1), K=2)
  pk('c3+1-pad8-hw1-src2-only', 3, 1, 8, 1, 'src2', (1, 0))
  pk('c3+1-pad4-hw257-c2-with-null-src2', 3, 1, 4, 257, 'c2_null', (0, 1), K=2)
  pk('c1+2-pad3-hw256-src', 1, 0, 3, 256, 'src', (0, 0))

  # ---- geeco_dynimg_bwd.  mins / maxs: per sample the element positions (of the HW * C run) that hold the extremum: one =
  # unique, several = a tie (copies of the first); kind 'flat': every frame constant; 'random': nothing planted.
  def dy(id, HW, C, mins=None, maxs=None, K=4, N=1, Cpad=None, two=False, outs='both', acc=(0, 0), lay=None, kind='planted', twin=False):
    kind = 'flat' if K == 1 else kind
    add('dynimg', id, HW=HW, C=C, K=K, N=N, Cpad=Cpad or (4 if C <= 4 else 8), two=two, outs=outs if two else 'd1', acc=acc,
        lay=dict(lay or {}), kind=kind, mins=mins, maxs=maxs, twin=twin)
  # instantiation: <4>, and <1> for each reason on its own (layout reasons: the same values through <4> as well)
  dy('v4-dense', 300, 4, [[5]], [[1100]])
  dy('v1-hwc75', 25, 3, [[3]], [[70]])
  two3 = dict(spad=800)      # the two-frame forms: frame t of an [N][3] stack (sample stride 3 HW C), as graph.py's pair_bwd
  for name, lay in (('sample_stride', dict(spad=2)), ('frame_stride', dict(fpad=1)), ('d_sample_stride', dict(dspad=2)),
                    ('d_frame_stride', dict(dfpad=1)), ('frames-off', dict(off=1)), ('d_frames-off', dict(doff=1))):
    dy('v1-by-' + name, 100, 3, [[7], [250]], [[260], [3]], N=2, lay=lay, twin=True)
  for name, lay in (('frames2-off', dict(off2=1)), ('d_frames2-off', dict(doff2=1))):
    dy('v1-by-' + name, 100, 4, [[7], [250]], [[260], [3]], K=2, N=2, two=True, lay=dict(two3, dspad=800, **lay), twin=True)
  # blocks: nblk in {1, 2, 5} for each V; exactly one block, one unit more, a ragged last block; where the extrema sit
  dy('v4-1block-exact-same-block', 256, 4, [[10]], [[1000]])
  dy('v4-one-unit-more-min-first-max-last', 257, 4, [[0]], [[1025]])
  dy('v4-5blocks-ragged-min-in-last', 1500, 3, [[4400]], [[2100]])
  dy('v1-1block-exact-same-block', 256, 1, [[10]], [[200]], Cpad=3, lay=dict(off=1))
  dy('v1-one-unit-more-min-first-max-last', 257, 1, [[0]], [[256]], Cpad=3)
  dy('v1-5blocks-ragged-min-in-last', 359, 3, [[1076]], [[600]])
  # ties
  dy('tie-2max-one-block', 300, 4, [[700]], [[10, 500]])
  dy('tie-2max-two-blocks', 300, 4, [[700]], [[10, 1100]])
  dy('tie-3min-three-blocks-v1', 359, 3, [[5, 300, 1076]], [[600]])
  dy('tie-3min-three-blocks-v4', 1500, 3, [[7, 2000, 4499]], [[3000]])
  dy('tie-both-over-blocks', 1500, 3, [[1, 4499]], [[1500, 3000, 3001]])
  dy('flat-v4', 300, 4, kind='flat', N=2)
  dy('flat-v1', 25, 3, kind='flat')
  dy('flat-acc', 300, 4, kind='flat', acc=(1, 0))
  # shapes
  dy('K1', 100, 3, K=1)
  dy('K1-acc', 100, 3, K=1, acc=(1, 0), N=2)
  dy('K2', 100, 3, [[7]], [[260]], K=2)
  dy('K3', 100, 3, [[7]], [[260]], K=3)
  dy('K3-acc', 99, 3, [[7]], [[260]], K=3, acc=(1, 0))
  dy('K16', 100, 3, [[7]], [[260]], K=16)
  dy('K64', 100, 3, [[7]], [[260]], K=DYN_MAXK)
  dy('K64-v1', 99, 3, [[290]], [[2]], K=DYN_MAXK)
  dy('C1-Cpad3', 260, 1, [[7]], [[250]], Cpad=3)
  dy('C2-Cpad4', 514, 2, [[7]], [[1026]], Cpad=4)
  dy('C3-Cpad8', 100, 3, [[7]], [[260]], Cpad=8)
  dy('C4-Cpad8', 300, 4, [[1100]], [[260]], Cpad=8)
  dy('C3-Cpad8-v1', 99, 3, [[7]], [[260]], Cpad=8)
  dy('N3-v4', 300, 4, [[5], [1100], [600]], [[1100], [5], [1150]], N=3)
  dy('N3-v1', 99, 3, [[5], [290], [100]], [[290], [5], [280]], N=3)
  for outs, acc in (('both', (0, 0)), ('d2', (0, 0)), ('d1', (0, 0)), ('both', (1, 0)), ('both', (0, 1)), ('both', (1, 1)), ('d2', (0, 1))):
    dy('two-%s-acc%d%d' % (outs, acc[0], acc[1]), 400, 3, [[7], [1100]], [[1150], [3]], K=2, N=2, two=True, outs=outs, acc=acc,
       lay=dict(spad=2400, dspad=2400))
  dy('two-v1-hwc75-acc11', 25, 3, [[7], [70]], [[60], [3]], K=2, N=2, two=True, acc=(1, 1), lay=dict(spad=150, dspad=150))
  # nothing planted: the recomputed extrema are the forward's (one case per V)
  dy('random-v4', 300, 4, kind='random', N=2)
  dy('random-v1', 99, 3, kind='random', N=2)
  return cases


CASES = _build()


# ---- the host side of each launch (input_grad.hip's entry points, restated) ------------------------------------------------
def conv1_geometry(c):
  """Group count and strides (floats), buffer lengths, and the tile grid of geeco_conv1_dgrad for the case."""
  F, H, W, Cin = c.F, c.H, c.W, c.Cin
  n_dz, n_w, n_dx = F * H * W * C1D_CO, 9 * Cin * C1D_CO, F * H * W * 4
  G = 1 if c.form == 'g1' else 2
  pad = (8, 4, 12) if c.form == 'padded' else (0, 0, 0)
  gs = [0, 0, 0] if G == 1 else [n_dz + pad[0], n_w + pad[1], n_dx + pad[2]]
  Gw = G
  if c.form == 'shared_w':
    gs[1], Gw = 0, 1
  return dict(G=G, Gw=Gw, gs_dz=gs[0], gs_w=gs[1], gs_dx=gs[2], n_dz=n_dz, n_w=n_w, n_dx=n_dx,
              len_dz=(G - 1) * gs[0] + n_dz, len_w=(Gw - 1) * gs[1] + n_w, len_dx=(G - 1) * gs[2] + n_dx,
              tiles_y=cdiv(H, C1D_TY), tiles_x=cdiv(W, C1D_TX), kernel='conv1_dgrad_valu<cin%d>' % Cin)


def dyn_geometry(c):
  """What geeco_dynimg_bwd's host code computes from the case: strides, ``vec`` (as the reasons against it), V, nblk, the
  workspace; and the index of every logical element inside each flat buffer (relative to the pointer the launch is given)."""
  N, K, total = c.N, c.K, c.HW * c.C
  lay = dict(fpad=0, spad=0, dfpad=0, dspad=0, off=0, doff=0, off2=0, doff2=0)
  lay.update(c.lay)
  has1, has2 = c.outs in ('both', 'd1'), c.two and c.outs in ('both', 'd2')
  if c.two:
    assert K == 2
    Kf, fs, dfs = 1, 0, 0
    ss, dss = total + lay['spad'], total + lay['dspad']
  else:
    Kf, fs, dfs = K, total + lay['fpad'], total + lay['dfpad']
    ss, dss = K * fs + lay['spad'], K * dfs + lay['dspad']
  reasons = set()
  for name, bad in (('total', total % 4), ('sample_stride', ss % 4), ('frame_stride', fs % 4), ('d_sample_stride', dss % 4),
                    ('d_frame_stride', dfs % 4), ('frames', lay['off']), ('d_frames', has1 and lay['doff']),
                    ('frames2', c.two and lay['off2']), ('d_frames2', has2 and lay['doff2'])):
    if bad:
      reasons.add(name)
  V = 1 if reasons else 4
  e = np.arange(total)
  idx = (np.arange(N) * ss)[:, None, None] + (np.arange(Kf) * fs)[None, :, None] + e
  didx = (np.arange(N) * dss)[:, None, None] + (np.arange(Kf) * dfs)[None, :, None] + e
  return dict(total=total, Kf=Kf, ss=ss, fs=fs, dss=dss, dfs=dfs, reasons=reasons, V=V, nblk=cdiv(total, 256 * V), has1=has1, has2=has2,
              ws_bytes=N * (cdiv(total, 256) + 1) * 8 * 4, rec_floats=N * cdiv(total, 256 * V) * 8, off=lay['off'], doff=lay['doff'],
              off2=lay['off2'], doff2=lay['doff2'], idx=idx, didx=didx, len_f=int(idx.max()) + 1, len_d=int(didx.max()) + 1,
              kernels=['dynimg_bwd_reduce_kernel<%d>' % V, 'dynimg_bwd_apply_kernel<%d>' % V])


def dense_twin(c):
  """The same values in the dense aligned layout: runs through <4> (for the <1> cases forced by layout alone)."""
  lay = dict(spad=c.lay['spad'], dspad=c.lay['spad']) if c.two else {}
  t = c.replace(lay=lay, twin=False, id=c.id + '-as-v4')
  assert dyn_geometry(t)['V'] == 4
  return t


# ---- inputs ----------------------------------------------------------------------------------------------------------------
def alpha64(K):
  return O.dynimg_alpha(K).astype(np.float64)


def _dyn_D(x, a):
  """D = sum_t a_t x_t and sum_t |a_t x_t| of one sample, x [K][total] float64: element-wise loops, so that elements holding the
  same values in every frame give the same D to the last bit."""
  D, absD = np.zeros(x.shape[1]), np.zeros(x.shape[1])
  for t in range(x.shape[0]):
    D += a[t] * x[t]
    absD += np.abs(a[t] * x[t])
  return D, absD


def _dyn_frames(c, seed):
  r = np.random.default_rng(seed)
  N, K, total = c.N, c.K, c.HW * c.C
  a = O.dynimg_alpha(K)
  frames = r.random([N, K, total], dtype=F32)
  g = r.standard_normal([N, total]).astype(F32)
  if c.kind == 'flat':
    frames[...] = r.random([N, K, 1], dtype=F32)
  elif c.kind == 'planted':
    for n in range(N):
      for pos, up in ((c.maxs[n], True), (c.mins[n], False)):
        for t in range(K):
          if a[t] != 0:
            frames[n, t, pos[0]] = HI if (a[t] > 0) == up else LO
          frames[n, t, pos] = frames[n, t, pos[0]]      # a tie = copies of the first element, in every frame
        g[n, pos] = g[n, pos[0]]                        # ... and of its g: the outputs of tied elements are bitwise equal
  return frames, g


def check_dyn_inputs(c, frames):
  """The input conditions, on the host before anything is launched: planted extrema at the positions the case names with
  MARGIN to the next distinct value in float64; tied elements bitwise equal in every frame; a flat sample constant per frame."""
  a = alpha64(c.K)
  for n in range(c.N):
    D, _ = _dyn_D(frames[n].astype(np.float64), a)
    vals = np.unique(D)
    if c.kind == 'flat':
      assert len(vals) == 1 and all(len(np.unique(frames[n, t].view(np.int32))) == 1 for t in range(c.K)), c.id
      continue
    assert vals[-1] - vals[-2] >= MARGIN and vals[1] - vals[0] >= MARGIN, (c.id, n)
    if c.kind == 'planted':
      assert sorted(np.flatnonzero(D == vals[0])) == sorted(c.mins[n]) and sorted(np.flatnonzero(D == vals[-1])) == sorted(c.maxs[n]), (c.id, n)
      for pos in (c.mins[n], c.maxs[n]):
        bits = frames[n][:, pos].view(np.int32)
        assert (bits == bits[:, :1]).all(), (c.id, n, 'tied elements differ in a frame')
    else:
      assert (D == vals[0]).sum() == 1 and (D == vals[-1]).sum() == 1, (c.id, n)


def input_grad_inputs(c):
  """The case's inputs, deterministic from its index (a 'random' dynimg case: the first seed of its sequence whose extrema
  keep MARGIN).  conv1: dz [G][F][H][W][32], w [Gw][3][3][Cin][32]; pack: g [N][HW][Cpad] (NaN in every channel the form does not
  read), a0 [N][K][HW][C1], b0 [N][K][HW][C2] (the start values); dynimg: frames [N][K][total], g [N][total], gp [N][HW][Cpad] (g
  with NaN in the unused channels), start [N][K][total]."""
  r = np.random.default_rng(7000 + c.index)
  if c.entry == 'conv1':
    geo = conv1_geometry(c)
    shape_dz, shape_w = [geo['G'], c.F, c.H, c.W, C1D_CO], [geo['Gw'], 3, 3, c.Cin, C1D_CO]
    if c.exact:      # |dz| <= 3, |w| <= 4: every product and every partial sum (<= 288 * 12) is an integer below 2^24
      dz, w = r.integers(-3, 4, shape_dz).astype(F32), r.integers(-4, 5, shape_w).astype(F32)
    else:
      dz = r.standard_normal(shape_dz).astype(F32)
      dz *= r.random(dz.shape) < 0.5                       # about half the entries zero, as after a ReLU gradient
      w = (r.standard_normal(shape_w) / np.sqrt(9 * C1D_CO)).astype(F32)
    return dict(dz=dz, w=w)
  if c.entry == 'pack':
    g = r.standard_normal([c.N, c.HW, c.Cpad]).astype(F32)
    lo, hi = (c.C1, c.C1 + c.C2) if c.form == 'src2' else (0, c.C1 + (c.C2 if c.form == 'both' else 0))
    g[..., :lo] = np.nan
    g[..., hi:] = np.nan
    return dict(g=g, a0=r.standard_normal([c.N, c.K, c.HW, c.C1]).astype(F32), b0=r.standard_normal([c.N, c.K, c.HW, max(c.C2, 1)]).astype(F32))
  for s in range(64):
    frames, g = _dyn_frames(c, 7000 + c.index + 1000 * s)
    if c.kind != 'random' or extrema_margin(frames) >= MARGIN:
      break
  check_dyn_inputs(c, frames)
  gp = np.full([c.N, c.HW, c.Cpad], np.nan, F32)
  gp[..., :c.C] = g.reshape(c.N, c.HW, c.C)
  return dict(frames=frames, g=g, gp=gp, start=r.standard_normal(frames.shape).astype(F32))


# ---- references, right and wrong ---------------------------------------------------------------------------------------------
CONV_MISTAKES = ('kx-mirrored', 'halo-column-zeroed')
DYN_MISTAKES = ('tie-n-minus-1', 'no-block-correction', 'minmax-swapped', 'alpha-neighbour', 'cpad4-for-8', 'ragged-unit-dropped',
                'ordinary-rel-1e-5')


def conv1_eval(c, inp, mistake=None):
  """dx [G][F][H][W][4] in float64 (channel 3 of an RGB layer: 0).  Mistakes: every tap mirrored in kx; the halo column at
  x0 - 1 of every tile but the first of a row read as zero (the kx = 2 tap of the columns x = 32, 64, ... is lost)."""
  geo = conv1_geometry(c)
  dx = np.zeros([geo['G'], c.F, c.H, c.W, 4])
  for g in range(geo['G']):
    w = inp['w'][g if geo['Gw'] > 1 else 0].astype(np.float64)
    if mistake == 'kx-mirrored':
      w = w[:, ::-1]
    dx[g][..., :c.Cin] = conv1_dgrad_ref(inp['dz'][g], w)
    if mistake == 'halo-column-zeroed':
      only = np.zeros_like(w)
      only[:, 2] = w[:, 2]
      dx[g][:, :, C1D_TX::C1D_TX, :c.Cin] -= conv1_dgrad_ref(inp['dz'][g], only)[:, :, C1D_TX::C1D_TX]
  return dx


def dyn_eval(c, inp, mistake=None, with_bounds=False):
  """d [N][K][total] in float64 by the formula of ``dynimg_bwd_ref`` (D formed element by element: see _dyn_D), or what a wrong
  kernel would give (DYN_MISTAKES); None when the mistake does not touch this case.  ``with_bounds``: (d, bound), bound per element.

  The bound, from input_grad.hip's own order of operations (every ^ is the float32 value):
    D^_j   K fused multiply-adds in t order: |D^_j - D_j| <= eD_j = gamma(K) sum_t |a_t x_tj|.  MARGIN is thousands of times that,
           so mn^ / mx^ sit where mn / mx sit: |mn^ - mn| <= e_mn = eD at the minimum (ties: the largest), e_mx likewise.
    r^     = fl(fl(mx^ - mn^) + 1e-6f): e_r = e_mn + e_mx + U (mx - mn) + U r + U 1e-6 (the constant's own rounding); rho = e_r / r.
           The flat sample: mx^ and mn^ are the SAME float, their difference is exactly 0, e_r = U r + U 1e-6 ("the same formula
           with r = 1e-6"), and every D^_j - mn^ below is exactly 0 as well (delta_j = 0).
    S^     sum g_j: <= V - 1 additions in the thread, 6 butterfly levels, 3 over the waves, nblk - 1 over the records:
           e_S = gamma(V + 9 + nblk) sum |g_j|   (counted generously: one per level a term can pass).
    T^     sum_b [T^_b + (mn^_b - mn^) S^_b], T^_b = sum g_j (D^_j - mn^_b): per term a subtraction and a product (2), the same tree
           (V + 9), the fold's subtraction, product and two additions (<= 4) per record over nblk records; the magnitudes of all
           terms add up to sum |g_j| (D^_j - mn^) (block part (D_j - mn_b) + correction part (mn_b - mn), both >= 0), and
           D^_j - mn^ <= (D_j - mn) + delta_j with delta_j = eD_j + e_mn:
           e_T = gamma(V + 14 + nblk) sum |g_j| (D_j - mn + delta_j)  +  sum |g_j| delta_j   (rounding; the data's own error).
    A^     = fl(T^ / r^): e_A = e_T / r + |A| (DIV_U U + rho)
    X^     = fl(fl(A^ / r^) / n_max), what a maximum gives:  e_X = e_A / (r n_max) + |X| (2 DIV_U U + rho)
    Y^     = fl(fl(fl(A^ - S^) / r^) / n_min), what a minimum takes: e_Y = (e_A + e_S) / (r n_min) + |Y| (U + 2 DIV_U U + rho)
           (n_min / n_max: sums of counts <= 1024 per block, exact in float32)
    dD^_i  = fl(g_i / r^), then + Y^ at a minimum, then - X^ at a maximum, one rounding each:
           e_dD = |g_i / r| (DIV_U U + rho) + [min] (e_Y + U |g_i / r + Y|) + [max] (e_X + U |dD_i|)
    out    = fl(a_t dD^_i): bound = (|a_t| e_dD + U |a_t dD_i|) SECOND.
  An ordinary element keeps the first term and the last: (DIV_U + 1) U |ref| plus what r's own error contributes.  The margin over
  the rounding counts is _primitive_refs' for its sums (colsum_bound, sumsq_rel_bound): factor 1 -- the count is a worst case with
  every rounding at its maximum and in the same direction, sqrt(count) above what a sum of that length typically shows."""
  geo = dyn_geometry(c)
  N, K, total, V, nblk = c.N, c.K, geo['total'], geo['V'], geo['nblk']
  a = alpha64(K)
  frames = inp['frames'].astype(np.float64)
  if mistake == 'cpad4-for-8':
    if c.Cpad != 8:
      return None
    flat = inp['gp'].reshape(-1)
    px, ch = np.divmod(np.arange(total), c.C)
    gs = np.stack([flat[(n * c.HW + px) * 4 + ch] for n in range(N)]).astype(np.float64)
  else:
    gs = inp['g'].astype(np.float64)
  out, bound, touched = np.zeros([N, K, total]), np.zeros([N, K, total]), False
  blk = np.arange(total) // (256 * V)
  for n in range(N):
    g = gs[n]
    D, absD = _dyn_D(frames[n], a)
    live = np.ones(total, bool)
    if mistake == 'ragged-unit-dropped' and total % (256 * V) and K > 1:
      live[total - V:] = False      # the reduction skips the last unit: its g and its D are in no record
      touched = True
    mn, mx = D[live].min(), D[live].max()
    r = mx - mn + 1e-6
    is_min, is_max = D == mn, D == mx
    nmin, nmax = float(is_min.sum()), float(is_max.sum())
    if mistake == 'tie-n-minus-1' and K > 1:
      touched = touched or nmin > 1 or nmax > 1
      nmin, nmax = max(nmin - 1, 1.0), max(nmax - 1, 1.0)
    S = (g * live).sum()
    if mistake == 'no-block-correction':
      mnb = np.array([D[blk == b].min() for b in range(nblk)])
      T = (g * (D - mnb[blk])).sum()
      touched = touched or (nblk > 1 and K > 1 and not (mnb == mn).all())
    else:
      T = (g * live * (D - mn)).sum()
    A = T / r
    Y, X = ((A - S) / r) / nmin, (A / r) / nmax
    if mistake == 'minmax-swapped':
      is_min, is_max = is_max, is_min
      touched = touched or (K > 1 and mn != mx)      # (the flat sample: every element is both)
    q = g / r
    p1 = q + is_min * Y
    dD = p1 - is_max * X
    if mistake == 'ordinary-rel-1e-5':
      dD = np.where(is_min | is_max, dD, dD * (1.0 + 1e-5))
      touched = touched or (K > 1 and not (is_min | is_max).all())
    at = np.roll(a, -1) if mistake == 'alpha-neighbour' else a
    touched = touched or (mistake == 'alpha-neighbour' and K > 1) or mistake == 'cpad4-for-8'
    out[n] = at[:, None] * dD
    if with_bounds:
      flat_sample = mn == mx
      eD = gamma(K) * absD
      e_mn, e_mx = (0.0, 0.0) if flat_sample else (eD[is_min].max(), eD[is_max].max())
      delta = np.zeros(total) if flat_sample else eD + e_mn
      e_r = e_mn + e_mx + U * (mx - mn) + U * r + U * 1e-6
      rho = e_r / r
      absg = np.abs(g)
      e_S = gamma(V + 9 + nblk) * absg.sum()
      e_T = gamma(V + 14 + nblk) * (absg * (D - mn + delta)).sum() + (absg * delta).sum()
      e_A = e_T / r + abs(A) * (DIV_U * U + rho)
      e_X = e_A / (r * nmax) + abs(X) * (2 * DIV_U * U + rho)
      e_Y = (e_A + e_S) / (r * nmin) + abs(Y) * (U + 2 * DIV_U * U + rho)
      e_dD = np.abs(q) * (DIV_U * U + rho) + is_min * (e_Y + U * np.abs(p1)) + is_max * (e_X + U * np.abs(dD))
      bound[n] = (np.abs(a)[:, None] * e_dD + U * np.abs(out[n])) * SECOND
  if mistake is not None and not touched:
    return None
  return (out, bound) if with_bounds else out


def dyn_split(c, d):
  """d [N][K][total] -> the outputs the case's form writes: 'd_frames' [N][Kf][total], 'd_frames2' [N][total] (two-frame form)."""
  geo = dyn_geometry(c)
  out = {}
  if geo['has1']:
    out['d_frames'] = d[:, :geo['Kf']]
  if geo['has2']:
    out['d_frames2'] = d[:, 1]
  return out


def input_grad_reference(c, inp):
  """{output name: dict(val float64, bound float64 per element, eq bool per element (equality with val asked for), ties [(sample,
  positions)] whose outputs must be bitwise equal)}.  conv1: 'dx' [G][F][H][W][4]; pack: 'd_src' [N][K][HW][C1] / 'd_src2' (the WHOLE
  stacks: the other frames keep their start values); dynimg: what ``dyn_split`` names, of the OVERWRITING form (an accumulating
  launch is start + that, one float32 addition: the GPU test checks it bitwise and compares the overwriting result)."""
  if c.entry == 'conv1':
    geo = conv1_geometry(c)
    val = conv1_eval(c, inp)
    # one fmaf chain of 9 * 32 terms per output, first into 0: term k passes at most 288 roundings -> gamma(288) sum |dz w|
    # (factor 1 over the count, as colsum_bound: see dyn_eval)
    bound = np.zeros_like(val)
    for g in range(geo['G']):
      bound[g][..., :c.Cin] = gamma(9 * C1D_CO) * conv1_dgrad_ref(np.abs(inp['dz'][g]), np.abs(inp['w'][g if geo['Gw'] > 1 else 0]))
    eq = np.zeros(val.shape, bool)
    eq[..., c.Cin:] = True      # the fourth channel of an RGB layer: exactly 0
    if c.exact:
      eq[...] = True
    return dict(dx=dict(val=val, bound=bound, eq=eq, ties=[]))
  if c.entry == 'pack':
    g, t = inp['g'], c.t
    a, b = inp['a0'].copy(), inp['b0'].copy()
    both = c.form == 'both'
    ra, rb = pack_bwd_ref(g, c.C1, d_src=a[:, t] if c.acc[0] else None, C2=c.C2 if c.form in ('both', 'src2') else 0,
                          d_src2=b[:, t, :, :c.C2] if c.acc[1] else None)
    ref = {}
    if c.form != 'src2':
      a[:, t] = ra
      ref['d_src'] = dict(val=a.astype(np.float64), bound=None, eq=np.ones(a.shape, bool), ties=[])
    if both or c.form == 'src2':
      b[:, t, :, :c.C2] = rb
    if c.C2:      # (c2_null: d_src2 is not passed, and the buffer keeps every start value)
      ref['d_src2'] = dict(val=b.astype(np.float64), bound=None, eq=np.ones(b.shape, bool), ties=[])
    return ref
  d, bound = dyn_eval(c, inp, with_bounds=True)
  a = alpha64(c.K)
  eq = np.zeros(d.shape, bool)
  eq[:, a == 0] = True        # K = 1 (alpha = [0]): all zeros; no other window length of the reference has a zero coefficient
  ties = []
  if c.kind == 'planted':
    ties = [(n, pos) for n in range(c.N) for pos in (c.mins[n], c.maxs[n]) if len(pos) > 1]
  vals, bounds, eqs = dyn_split(c, d), dyn_split(c, bound), dyn_split(c, eq)
  return {k: dict(val=vals[k], bound=bounds[k], eq=eqs[k], ties=ties) for k in vals}


def input_grad_compare(c, got, ref):
  """-> ({output: worst err / bound}, [problems]).  No NaN in any output; equality where the case asks for it (the integer case,
  the pack adjoint, the K = 1 frames, channel 3 of an RGB conv1, the bit-equal outputs of tied elements); every other element under
  its own bound."""
  worst, problems = {}, []
  if sorted(got) != sorted(ref):
    return worst, ['outputs %s, expected %s' % (sorted(got), sorted(ref))]
  for name, r in ref.items():
    x = np.asarray(got[name])
    val, eq = r['val'], r['eq']
    if x.shape != val.shape:
      problems.append('%s: shape %s, expected %s' % (name, x.shape, val.shape))
      continue
    if np.isnan(x).any():
      problems.append('%s: %d NaN' % (name, int(np.isnan(x).sum())))
      continue
    x64 = x.astype(np.float64)
    ne = eq & (x64 != val)
    if ne.any():
      at = tuple(int(v) for v in np.argwhere(ne)[0])
      problems.append('%s: %d elements differ where equality is asked, first at %s: %.9g != %.9g' % (name, int(ne.sum()), at, x64[at], val[at]))
    worst[name] = 0.0
    if r['bound'] is not None and not eq.all():
      err, b = np.abs(x64 - val)[~eq], r['bound'][~eq]
      share = np.where(err == 0, 0.0, err / np.maximum(b, 1e-300))
      worst[name] = float(share.max())
      if (share > 1).any():
        k = int(share.argmax())
        at = tuple(int(v) for v in np.argwhere(~eq)[k])
        problems.append('%s: %d of %d elements out of bound; worst at %s: got %.9g, reference %.9g, err %.3e (bound %.3e)' % (
            name, int((share > 1).sum()), share.size, at, x64[at], val[at], err[k], b[k]))
    for n, pos in r['ties']:
      bits = np.ascontiguousarray(x[n].reshape(-1, x.shape[-1])[:, pos]).view(np.int32)
      if not (bits == bits[:, :1]).all():
        problems.append('%s: the tied elements %s of sample %d differ' % (name, list(pos), n))
  return worst, problems
