"""HBM-resident episodes: an episode's frames are uploaded once (``episode_to_device``, kept across epochs by ``EPISODE_CACHE``)
and a batch of K-frame windows is a ``DeviceWindows``, which the feed (feed.py) turns into addresses or gathers in HBM.  The
reader that builds them is input_fn.py; it re-exports every name of this module."""
import collections
import os
import threading

import numpy as np


def resolve_device(device):
  """An explicit (type, index) device.  A bare 'cuda' means the CALLING thread's current device: resolve it
  before handing work to another thread (the current HIP device is thread-local and starts at 0 there)."""
  import torch
  d = torch.device(device)
  if d.type == 'cuda' and d.index is None:
    d = torch.device('cuda', torch.cuda.current_device())
  return d


class WindowAugment:
  """The per-window augmentation draws of ONE batch (pickplace_input_fn(augment=...)): ``shift`` int32 [n][2] =
  (dy, dx) in whole pixels, ``colour`` float32 [n][6] = gain[3], bias[3] of the RGB channels.  One object is referenced by every
  DeviceWindows stream of the batch (``DeviceWindows.augment``): window i of 'rgb', 'target_rgb', 'depth' and 'target_depth'
  moves by the same shift[i], the RGB streams are tinted by the same colour[i], depth streams are only moved.
  The scene extras (RGB streams only, each optional): ``occ_rect`` int32 [n][4][4] = (y0, x0, h, w) of up to four
  rectangles per window in output coordinates with ``occ_colour`` float32 [n][4][3] (an all-zero slot is empty), and the sensor
  noise ``sigma`` in (0, 1) with ``noise_key``, the two uint32 words of the batch's Philox key.
  The time extra (optional): ``frame_src`` int32 [n][K], the recorded frame each slot of window i shows as an offset
  from the window's start (None or arange(K): K consecutive frames).  Only the camera streams of the observation follow it
  (``DeviceWindows.timed``: 'rgb' and 'depth'); with zero shifts and the neutral colour row (gain 1, bias 0) it is all the object
  carries."""

  def __init__(self, shift, colour, occ_rect=None, occ_colour=None, noise_key=None, sigma=0.0, frame_src=None):
    self.shift = np.ascontiguousarray(shift, np.int32).reshape(-1, 2)
    self.colour = np.ascontiguousarray(colour, np.float32).reshape(-1, 6)
    if len(self.shift) != len(self.colour):
      raise ValueError('WindowAugment: %d shifts for %d colour rows' % (len(self.shift), len(self.colour)))
    if (occ_rect is None) != (occ_colour is None):
      raise ValueError('WindowAugment: occ_rect and occ_colour come together')
    self.occ_rect = self.occ_colour = self.noise_key = None
    if occ_rect is not None:
      self.occ_rect = np.ascontiguousarray(occ_rect, np.int32).reshape(-1, 4, 4)
      self.occ_colour = np.ascontiguousarray(occ_colour, np.float32).reshape(-1, 4, 3)
      if not len(self.occ_rect) == len(self.occ_colour) == len(self.shift):
        raise ValueError('WindowAugment: %d / %d occluder rows for %d windows' % (len(self.occ_rect), len(self.occ_colour), len(self.shift)))
    self.sigma = float(sigma)
    if not 0.0 <= self.sigma < 1.0:
      raise ValueError('WindowAugment: sigma must lie in [0, 1), got %r' % (sigma,))
    if self.sigma > 0:
      if noise_key is None:
        raise ValueError('WindowAugment: sigma > 0 needs a noise key')
      self.noise_key = np.ascontiguousarray(noise_key, np.uint32).reshape(2)
    self.frame_src = None
    if frame_src is not None:
      self.frame_src = np.ascontiguousarray(frame_src, np.int32)
      if self.frame_src.ndim != 2 or len(self.frame_src) != len(self.shift):
        raise ValueError('WindowAugment: frame_src of shape %s for %d windows' % (self.frame_src.shape, len(self.shift)))

  def __len__(self):
    return len(self.shift)

  @property
  def scene(self):
    """None, or which extras the draws carry: 'occlude', 'noise' or 'occlude+noise' (a feed slot is built for one of them)."""
    return '+'.join(w for w, on in (('occlude', self.occ_rect is not None), ('noise', self.noise_key is not None)) if on) or None


SCENE_TAGS = {'rgb': 0, 'target_rgb': 1}      # the noise generator's stream number of an RGB feature (counter word 3)
TIMED_KEYS = ('rgb', 'depth')      # the features whose slots follow WindowAugment.frame_src: the camera delivers both together


class DeviceWindows:
  """A batch of K-frame windows that lives in HBM as (episode frames, start indices) segments.

  Stands in for a dense [n, K, *frame_shape] float32 array in the features dict: the Estimator
  materialises it straight into the model's static input buffer with geeco_gather_windows (frames
  were uploaded once per episode, RGB as uint8), so no window ever crosses PCIe."""

  def __init__(self, K, frame_shape, divisor, squeeze_k=False):
    self.K, self.frame_shape, self.divisor, self.squeeze_k = K, tuple(frame_shape), float(divisor), squeeze_k
    self.segments = []      # (device tensor [T, frame_elems], np.int32 starts, divisor of THIS segment's frames)
    self.n = 0
    self.scattered = False  # built by the shuffling assembler (shuffle_windows): about one episode per window, see window_table
    self.augment = None     # a WindowAugment shared with the other streams of the batch: the windows are these, transformed
    self.scene_tag = 0      # SCENE_TAGS of the feature this stream is (the sensor noise of 'rgb' and 'target_rgb' differs)
    self.timed = False      # a camera stream of the observation (TIMED_KEYS): its slots follow ``augment.frame_src``

  def add(self, frames_dev, starts, divisor=None):
    """``divisor``: what the gather divides this segment's frames by (default: the constructor's).  One batch can hold
    episodes stored as uint8 (255) next to episodes kept as float32 (1): a batch that straddles two such episodes is
    gathered segment by segment with each one's own divisor (and is then not ``is_u8()``: dense path)."""
    starts = np.asarray(starts, np.int32)
    self.segments.append((frames_dev, starts, self.divisor if divisor is None else float(divisor)))
    self.n += len(starts)

  @property
  def shape(self):
    return (self.n,) + (() if self.squeeze_k else (self.K,)) + self.frame_shape

  augmented = property(lambda self: self.augment is not None)

  def augment_tables(self):
    """(shift int32 [n][2], colour float32 [n][6] or None) for ops.gather_windows_augmented_into: colour for RGB frames only
    (a one-channel stream is moved, never tinted)."""
    aug = self.augment
    if len(aug) != self.n:
      raise ValueError('DeviceWindows: augmentation draws for %d windows on a batch of %d' % (len(aug), self.n))
    if self.frame_shape[-1] not in (1, 3) or len(self.frame_shape) != 3:
      raise ValueError('DeviceWindows: augmented frames must be [H, W, 3] or [H, W, 1], got %s' % (self.frame_shape,))
    return aug.shift, (aug.colour if self.frame_shape[-1] == 3 else None)

  def scene_tables(self):
    """None (the draws carry no extras, or this is a one-channel stream: shift only, through the merged entry point), or
    (occ_rect int32 [n][4][4] or None, occ_colour float32 [n][4][3] or None, noise_key int32 [2] or None, sigma, tag) for
    ops.gather_windows_scene_into."""
    aug = self.augment
    if aug is None or aug.scene is None or self.frame_shape[-1] != 3:
      return None
    key = None if aug.noise_key is None else aug.noise_key.view(np.int32)
    return aug.occ_rect, aug.occ_colour, key, aug.sigma, self.scene_tag

  @property
  def frame_src(self):
    """int32 [n][K] frame offsets of this stream's slots, or None: the windows are K consecutive frames."""
    return self.augment.frame_src if self.augment is not None and self.timed else None

  def __len__(self):
    return self.n

  @staticmethod
  def concat(*parts):
    """The windows of ``parts`` in order; ``scattered`` when one of them is."""
    a = parts[0]
    out = DeviceWindows(a.K, a.frame_shape, a.divisor, a.squeeze_k)
    for b in parts:
      if (a.K, a.frame_shape, a.squeeze_k) != (b.K, b.frame_shape, b.squeeze_k):
        raise ValueError('DeviceWindows.concat: windows of different shapes (%s, %s)' % (a.shape[1:], b.shape[1:]))
      out.segments += b.segments
      out.n += b.n
      out.scattered = out.scattered or b.scattered
      if b.augment is not None:
        raise ValueError('DeviceWindows.concat: augmented windows (the draws belong to one emitted batch)')
    return out

  def is_u8(self):
    """Every segment is resident uint8 frames (the recorder's values; the consumer divides by 255)."""
    import torch
    return bool(self.segments) and all(
        f is not None and d == 255.0 and f.dtype == torch.uint8 and f.is_contiguous() for f, _, d in self.segments)

  def _checked_segments(self, device, who=None):
    """The ONE walk over the segments: per segment (frames, int32 starts, divisor, kind, bytes per frame), once its frames are
    known to be uploaded, to live on ``device`` (None: not checked here) and to hold every window of ``starts``.  ``who`` names
    a caller that follows addresses; its kernels convert two kinds of frames, 'u8' (uint8, divisor 255) and 'f32' (float32,
    divisor 1), and anything else raises.  Without ``who`` kind and bytes are None (the per-segment gather takes any divisor)."""
    import torch
    fe = int(np.prod(self.frame_shape))
    kinds = {(torch.uint8, 255.0): ('u8', fe), (torch.float32, 1.0): ('f32', 4 * fe)}
    for frames_dev, starts, divisor in self.segments:
      if frames_dev is None:
        raise RuntimeError('DeviceWindows: this image stream was not uploaded (device_keys excluded it)')
      if device is not None and frames_dev.device != device:
        raise RuntimeError('DeviceWindows: episode frames live on %s but are read on %s (each rank must upload to its '
                           'own GPU)' % (frames_dev.device, device))
      T = frames_dev.shape[0]
      if len(starts) and (int(starts.min()) < 0 or int(starts.max()) + self.K > T):
        raise IndexError('DeviceWindows: window [%d, %d) outside the %d resident frames' %
                         (int(starts.min()), int(starts.max()) + self.K, T))
      if who and (frames_dev.dtype, divisor) not in kinds:
        raise ValueError('DeviceWindows.%s: frames of type %s with divisor %g are neither the uint8 (255) nor the '
                         'float32 (1) form' % (who, frames_dev.dtype, divisor))
      yield (frames_dev, starts, divisor) + (kinds[frames_dev.dtype, divisor] if who else (None, None))

  def _window_addresses(self, device, who):
    """(int64 [n] address of each window's first frame, int32 [n] kind: 0 = uint8 frames / 1 = float32 frames, int64 [n] bytes
    per frame), after the checks of ``_checked_segments``."""
    addr, kinds, stride = np.empty(self.n, np.int64), np.empty(self.n, np.int32), np.empty(self.n, np.int64)
    off = 0
    for frames_dev, starts, _, kind, frame_bytes in self._checked_segments(device, who):
      sl = slice(off, off + len(starts))
      addr[sl] = frames_dev.data_ptr() + starts.astype(np.int64) * frame_bytes
      kinds[sl], stride[sl] = kind == 'f32', frame_bytes
      off += len(starts)
    return addr, kinds, stride

  def addresses(self, device):
    """int64 address of each window's first frame (WindowFeed.pointers(): the input kernel that follows them reads uint8 frames,
    so any other segment raises)."""
    if self.augment is not None:
      raise ValueError('DeviceWindows.addresses: augmented windows exist only as dense windows (the kernel that follows these '
                       'addresses reads the frames as recorded)')
    addr, kinds, _ = self._window_addresses(resolve_device(device), 'addresses')
    if kinds.any():
      raise ValueError('DeviceWindows.addresses: float32 frames, the kernel that follows these addresses reads the uint8 (255) form')
    return addr

  def window_table(self, device):
    """(addresses int64 [n], kinds int32 [n]) for ops.gather_windows_by_address_into: the address of each window's first frame
    and 0 for uint8 frames (divisor 255) / 1 for float32 frames (divisor 1).  One table may mix the two kinds.  Residency,
    bounds and device checks as ``addresses``."""
    return self._window_addresses(resolve_device(device), 'window_table')[:2]

  def frame_addresses(self, device):
    """(addresses int64 [n][K], kinds int32 [n]) for ops.gather_windows_frames_into: slot k of window i shows the frame
    ``max(start_i + frame_src[i][k], 0)`` of its episode (clamped at the episode's first frame, where the scene is at rest);
    without ``frame_src`` the consecutive table, ``window_table`` spread over K.  EVERY resulting frame index is checked against
    the segment's resident frames here, on the host, before anything is queued (IndexError): an out-of-range gather is a GPU
    fault.  uint8 frames may lie at any address, float32 frames must be 4-byte aligned.  Residency, kind and device checks as
    ``window_table``."""
    src = self.frame_src
    if src is None:
      src = np.broadcast_to(np.arange(self.K, dtype=np.int32), (self.n, self.K))
    if src.shape != (self.n, self.K):
      raise ValueError('DeviceWindows.frame_addresses: frame_src of shape %s on %d windows of %d frames' % (src.shape, self.n, self.K))
    addr, kinds = np.empty((self.n, self.K), np.int64), np.empty(self.n, np.int32)
    off = 0
    for frames_dev, starts, _, kind, frame_bytes in self._checked_segments(resolve_device(device), 'frame_addresses'):
      sl = slice(off, off + len(starts))
      idx = np.maximum(starts.astype(np.int64)[:, None] + src[sl].astype(np.int64), 0)
      T = frames_dev.shape[0]
      if idx.size and int(idx.max()) >= T:
        raise IndexError('DeviceWindows.frame_addresses: frame %d outside the %d resident frames' % (int(idx.max()), T))
      if kind == 'f32' and frames_dev.data_ptr() % 4:
        raise ValueError('DeviceWindows.frame_addresses: float32 frames at an address that is no multiple of 4')
      addr[sl] = frames_dev.data_ptr() + idx * frame_bytes
      kinds[sl] = kind == 'f32'
      off += len(starts)
    return addr, kinds

  def frame_table(self, capacity, targets=None, device=None):
    """The batch's DISTINCT frames, each once (shared-frame training, graph.py ``shared_frames``): returns
    (addresses int64 [capacity], index int32 [n][K], target_index int32 [n] or None, used).  ``addresses[index[n][t]]`` is the
    address of window n's frame t and ``addresses[target_index[n]]`` that of window n's frame of ``targets`` (a K = 1
    DeviceWindows of the same batch, e.g. 'target_rgb'); slots are numbered in first-use order -- this stream's windows row by
    row, then the targets -- across segments and across the two streams, and the table is zero-padded to ``capacity``
    (0 = unused slot).  Residency and device checks as ``addresses`` (``device`` None: the segments must share one device).
    Raises ValueError when the batch mixes uint8 and float32 episodes (the pack kernel takes one kind per call) or needs more
    than ``capacity`` slots."""
    if device is not None:
      device = resolve_device(device)
    streams = [self] if targets is None else [self, targets]
    if any(dw.augment is not None for dw in streams):
      raise ValueError('DeviceWindows.frame_table: augmented windows share no frames (each window is transformed by its own draw)')
    if targets is not None and (targets.n, targets.K, targets.frame_shape) != (self.n, 1, self.frame_shape):
      raise ValueError('DeviceWindows.frame_table: targets must be %d single frames of shape %s' % (self.n, self.frame_shape))
    devices = {f.device for dw in streams for f, _, _ in dw.segments if f is not None}
    if device is None and len(devices) > 1:
      raise RuntimeError('DeviceWindows: episode frames live on several devices (%s)' % sorted(map(str, devices)))
    addr, kinds = [], set()
    for dw in streams:      # every frame of every window: first frame + t frames on
      a, k, stride = dw._window_addresses(device, 'frame_table')
      addr.append((a[:, None] + np.arange(dw.K, dtype=np.int64)[None, :] * stride[:, None]).ravel())
      kinds |= set(k.tolist())
    if len(kinds) > 1:
      raise ValueError('DeviceWindows.frame_table: the batch mixes uint8 and float32 episodes (one frame kind per table)')
    flat = np.concatenate(addr)
    uniq, first, inv = np.unique(flat, return_index=True, return_inverse=True)
    order = np.argsort(first, kind='stable')          # distinct addresses by first use
    used = len(uniq)
    if used > capacity:
      raise ValueError('DeviceWindows.frame_table: the batch holds %d distinct frames, the table has capacity %d' % (used, capacity))
    slot = np.empty(used, np.int32)
    slot[order] = np.arange(used, dtype=np.int32)
    index = slot[inv.ravel()]
    table = np.zeros(capacity, np.int64)
    table[:used] = uniq[order]
    nk = self.n * self.K
    return table, index[:nk].reshape(self.n, self.K), (index[nk:].copy() if targets is not None else None), used

  def materialize_into(self, out):
    """out [n][K][*frame_shape] <- the windows, one geeco_gather_windows launch per segment.  Every segment is checked on the
    host (residency, device, bounds) before the first launch is queued: an out-of-range gather is a GPU fault.  Augmented
    windows: ONE launch (``_gather_by_tables``) behind small copies of the tables the draws carry (the feed's 'dense_augmented'
    and 'dense_frames' forms send them in the step's one block instead)."""
    import torch
    from . import ops
    fe = int(np.prod(self.frame_shape))
    if self.augment is not None:
      shift, colour = self.augment_tables()
      per_frame = self.frame_src is not None
      addr, kinds = self.frame_addresses(out.device) if per_frame else self.window_table(out.device)
      occ_rect, occ_colour, key, sigma, tag = self.scene_tables() or (None, None, None, 0.0, self.scene_tag)
      up = lambda a: None if a is None else torch.from_numpy(a).to(out.device, non_blocking=True)
      _gather_by_tables(out, [up(a) for a in (addr, kinds, shift, colour, occ_rect, occ_colour, key)], sigma, tag, per_frame,
                        self.n, self.K, self.frame_shape)
      return
    off = 0
    for frames_dev, starts, divisor, _, _ in list(self._checked_segments(out.device)):
      n = len(starts)
      st = torch.as_tensor(starts).to(out.device, non_blocking=True)
      ops.gather_windows_into(out[off:off + n], frames_dev, st, n, self.K, fe, divisor)
      off += n

  def numpy(self):
    """Dense host copy (tests / debugging)."""
    import torch
    dev = self.segments[0][0].device
    out = torch.empty((self.n, self.K) + self.frame_shape, dtype=torch.float32, device=dev)
    self.materialize_into(out)
    torch.cuda.synchronize()
    arr = out.cpu().numpy()
    return arr[:, 0] if self.squeeze_k else arr


def _gather_by_tables(out, tables, sigma, tag, per_frame, n, K, frame_shape):
  """out [n][K][*frame_shape] <- ONE launch of the gather that serves ``tables`` = (addr, kind, shift, colour, occ_rect, occ_colour,
  noise_key) on ``out``'s device, the last five None where the batch carries none: ops.gather_windows_frames_into when ``addr``
  holds one address per frame (``per_frame``), else _scene_into with extras, _augmented_into with a shift, _by_address_into
  without.  ``sigma`` and ``tag`` go to the first two.  The ONE place that answers this, for ``DeviceWindows.materialize_into``
  (tables uploaded) and ``WindowFeed.after_flush`` (views of the arena); the wrapper is looked up on ``ops`` when called."""
  from . import ops
  addr, kind, shift, colour, occ_rect, occ_colour, noise_key = tables
  if per_frame:
    ops.gather_windows_frames_into(out, *tables, sigma, tag, n, K, *frame_shape)
  elif occ_rect is not None or noise_key is not None:
    ops.gather_windows_scene_into(out, *tables, sigma, tag, n, K, *frame_shape)
  elif shift is not None:
    ops.gather_windows_augmented_into(out, addr, kind, shift, colour, n, K, *frame_shape)
  else:
    ops.gather_windows_by_address_into(out, addr, kind, n, K, int(np.prod(frame_shape)))


# ---- staging memory and the HBM-resident episode cache of the device path ----------------------------------------------
class _PinnedPool:
  """Page-locked staging arrays for the reader threads (the native reader writes the uint8 frames straight into
  them; the upload is then one DMA).  Blocks are recycled: pinning 20 MB costs more than reading it."""

  def __init__(self):
    self._free = collections.defaultdict(list)
    self._lock = threading.Lock()

  def take(self, nbytes):
    import torch
    from .runtime import CAPTURE_LOCK
    with self._lock:
      if self._free[nbytes]:
        return self._free[nbytes].pop()
    with CAPTURE_LOCK:       # hipHostMalloc must not fall into the training thread's capture window
      return torch.empty(nbytes, dtype=torch.uint8, pin_memory=True)

  def give(self, t):
    with self._lock:
      if len(self._free[t.numel()]) < 32:
        self._free[t.numel()].append(t)


_PINNED = _PinnedPool()


class EpisodeCache:
  """Episodes that stay in HBM across epochs: uint8 RGB frames (19.7 MB per 100-frame 256 x 256 episode; float32 depth
  26 MB more when the model reads it) + the few KB of per-frame states on the host.  Keyed by (file identity, device,
  streams held); filled first-come until ``budget_bytes`` of device memory are in use — no eviction: an epoch scans
  the dataset cyclically, where evicting the least recently used entry would always evict the next one needed.
  Epochs >= 2 then touch neither the disk nor PCIe for cached episodes (MI355X: 288 GB holds ~10 k RGB episodes)."""

  def __init__(self, budget_bytes=None):
    self.budget_bytes = budget_bytes      # None: 60 % of the device's memory, decided on first use
    self._entries = {}
    self._bytes = 0
    self._lock = threading.Lock()
    self.hits = self.misses = 0

  @staticmethod
  def key(path, device, fetch_target, image_keys):
    st = os.stat(path)
    return (os.path.realpath(path), st.st_size, st.st_mtime_ns, str(device), bool(fetch_target), tuple(sorted(image_keys)))

  def get(self, key):
    with self._lock:
      e = self._entries.get(key)
      if e is None:
        self.misses += 1
      else:
        self.hits += 1
      return e

  def put(self, key, ex, dev, device):
    import torch
    nbytes = sum(v.numel() * v.element_size() for v in dev.values() if hasattr(v, 'numel'))
    with self._lock:
      if self.budget_bytes is None:
        self.budget_bytes = int(0.6 * torch.cuda.get_device_properties(device).total_memory)
      if key in self._entries or self._bytes + nbytes > self.budget_bytes:
        return False
      self._entries[key] = (ex, dev)
      self._bytes += nbytes
      return True

  def clear(self):
    with self._lock:
      self._entries.clear()
      self._bytes = 0
      self.hits = self.misses = 0

  @property
  def bytes_in_use(self):
    return self._bytes

  def __len__(self):
    return len(self._entries)


EPISODE_CACHE = EpisodeCache()


def episode_to_device(ex, device, image_keys=('rgb', 'depth')):
  """Uploads the image streams of one episode (``load_episode(raw_rgb=True)``): RGB as uint8 when the recorded
  values were integral, depth as float32.  Returns (states, dev): ``states`` = ``ex`` without the image arrays (what
  the cache keeps on the host), ``dev`` = device tensors + the divisors the window gather applies."""
  import torch
  from .runtime import CAPTURE_LOCK
  device = resolve_device(device)
  T = ex['step'].shape[0]
  dev, host = {}, {}

  def stage(arr, rows):
    if arr.dtype == np.uint8:
      return torch.from_numpy(arr.reshape(rows, -1)), 255.0
    return torch.from_numpy(np.ascontiguousarray(arr.reshape(rows, -1) / np.float32(255.0))), 1.0

  if 'rgb' in image_keys:
    host['rgb'], dev['rgb_div'] = stage(ex['rgb'], T)
    if 'target_rgb' in ex:
      host['target_rgb'], dev['target_rgb_div'] = stage(ex['target_rgb'], 1)
  if 'depth' in image_keys:
    host['depth'] = torch.from_numpy(np.ascontiguousarray(ex['depth'].reshape(T, -1)))
    if 'target_depth' in ex:
      host['target_depth'] = torch.from_numpy(np.ascontiguousarray(ex['target_depth'].reshape(1, -1)))
  # allocations / synchronous copies from this (prefetch) thread must not fall into a hipGraph capture window of
  # the training thread (runtime.CAPTURE_LOCK)
  with CAPTURE_LOCK:
    for k, v in host.items():
      dev[k] = v.to(device)
  states = {k: v for k, v in ex.items() if k not in ('rgb', 'depth', 'target_rgb', 'target_depth')}
  states['_hw'] = ex['rgb'].shape[1:3]
  return states, dev
