"""Host models of the predictor I/O kernels (csrc/predict_io.hip), in numpy alone: what each entry point has to give, restated from
the batch-1 predictor the kernels stand for (reference src/models/e2evmc/predictor.py:127-209) and not from the kernels.

* range_flags: the frame check (predictor.py:134-138: np.amin / np.amax of the frame inside [0 - TOL, 1 + TOL]; a NaN turns both
  into NaN and every comparison false), per env, over channels 0..2 (the depth plane of an RGB-D frame is metres, not [0, 1]:
  geeco_amd/predictor.py:41), as the control words ctl [B + 1] the device keeps: ctl[b] per env, ctl[B] = any.
* the frame windows: WindowModel of tests/test_batched_predictor_cpu.py (held to predictor.py:144-146, 192-200 there), re-exported.
* pack_preds: the returned heads side by side; the gripper logits as float32(np.argmax(logits) - 1) (predictor.py:183-189).
* pack_images: the channel-padded debug images [B][HW][4] as [n][B][HW][C], in the order of the images given.
* the feature rings: FeatureRingModel of tests/test_incremental_predictor_cpu.py; that module needs torch for its other tests, so
  the GPU cases import the class from there and this module stays numpy-only.

tests/test_predict_io_ref_cpu.py tests these on hand-written cases; tests/test_predict_io_variants_gpu.py compares every launch
variant of predict_io.hip against them bit for bit.
"""
import numpy as np

from test_batched_predictor_cpu import WindowModel      # noqa: F401  (the one window model; re-exported)


def range_flags(frames, C, lo, hi, ctl=None):
  """frames [B][...][C] float32 -> int32 [B + 1]: word b = 1 when a value of channels 0..2 of env b is not inside [lo, hi] in
  float64 (a NaN is not), word B = 1 when any word is; OR-ed into ``ctl`` (the words of an earlier check) when given."""
  f = np.asarray(frames)
  B = f.shape[0]
  v = f.reshape(B, -1, C)[:, :, :3].astype(np.float64)
  inside = (v >= float(lo)) & (v <= float(hi))          # False for NaN
  bad = ~inside.reshape(B, -1).all(axis=1)
  out = np.zeros(B + 1, np.int32) if ctl is None else np.array(ctl, np.int32)
  assert out.shape == (B + 1,)
  out[:B] |= bad.astype(np.int32)
  out[B] |= np.int32(bad.any())
  return out


def pack_width(segs):
  """Output columns of a segment list of (src column, length, argmax)."""
  return sum(1 if am else n for _, n, am in segs)


def pack_preds(preds, segs):
  """preds [B][P] float32 -> [B][F] float32: per segment (src, len, argmax), in order, either the len columns from src or ONE
  column float32(np.argmax(columns) - 1)."""
  p = np.asarray(preds, np.float32)
  cols = []
  for src, n, am in segs:
    q = p[:, src:src + n]
    assert q.shape[1] == n, (src, n, p.shape)
    if am:
      cols.append(np.array([np.float32(np.argmax(row) - 1) for row in q], np.float32)[:, None])
    else:
      cols.append(q)
  return np.concatenate(cols, axis=1)


def pack_images(imgs, C):
  """imgs: the images of one call, each [B][HW][4] float32 or None -> [n][B][HW][C] over the n given ones, in their order."""
  given = [np.asarray(im, np.float32)[:, :, :C] for im in imgs if im is not None]
  return np.stack(given) if given else None


def newest_input(frames, C):
  """frames [B][HW][C] (float32, or uint8 RGB: float32(u8) / float32(255), tests/test_batched_predictor_cpu.py::
  test_uint8_division_is_the_float_path_exhaustively) -> the encoder input [B][HW][4]: a zero fourth channel for RGB, depth there
  for RGB-D."""
  f = np.asarray(frames)
  v = f.astype(np.float32) / np.float32(255.0) if f.dtype == np.uint8 else f
  out = np.zeros(f.shape[:2] + (4,), np.float32)
  out[:, :, :C] = v
  return out
