"""The per-step feed: how a batch reaches the static buffers a captured step reads.  ``build_slots`` makes one slot per feature /
label of a model's first batch: small host arrays share the ``FeedArena``, windows of HBM-resident episodes get a ``WindowFeed``,
anything else a device tensor of its own.  The model_fn adopts slots as its inputs, ``adopted_slots`` drops the rest, and per step
``feed_step`` runs, in the order graph replay depends on: arena ``begin``, every ``write`` / ``WindowFeed.feed``, one ``flush``,
then the ``after_flush`` launches.  input_fn.py re-exports ``FeedArena`` and ``WindowFeed``."""
import collections

import numpy as np

from .device_windows import DeviceWindows, _gather_by_tables, resolve_device

ARENA_MAX_BYTES = 1 << 20      # host arrays up to this size share the arena's one copy; larger ones (dense windows) go alone


class FeedArena:
  """Every per-batch host array of a model's feed (states, labels, window address tables) in ONE device block, written
  through ONE pinned staging block and ONE H2D copy per step: half a dozen small copies queued between two graph replays
  cost the host ~70 us per step, one ~30.  ``reserve`` while building, then ``seal``; per batch ``begin`` / ``write``... /
  ``flush``.  A ring of staging blocks lets the host run ahead: a block is rewritten only after its upload has finished.
  (Measured and not kept: uploading on a side stream into device-side landing blocks and moving them into place with a
  device-to-device copy - no gain; one small command between two replays of the step costs 6-10 us whatever it is,
  scripts/dev/between_graphs.py.)"""

  SLOTS = 4
  ALIGN = 256

  def __init__(self, device):
    self.device = resolve_device(device)      # indexed (a bare 'cuda' never compares equal to a tensor's cuda:N)
    self._layout = {}       # key -> (offset, nbytes, np dtype, shape)
    self._size = 0
    self.block = None
    self._open = False
    self._turn = 0

  def reserve(self, key, shape, dtype):
    if self.block is not None:
      raise RuntimeError('FeedArena.reserve after seal')
    dt = np.dtype(dtype)
    nbytes = int(np.prod(shape, dtype=np.int64)) * dt.itemsize
    self._layout[key] = (self._size, nbytes, dt, tuple(shape))
    self._size += -(-max(nbytes, 1) // self.ALIGN) * self.ALIGN

  def seal(self):
    import torch
    self.block = torch.zeros(max(self._size, self.ALIGN), dtype=torch.uint8, device=self.device)
    self._stage = [torch.zeros(self.block.numel(), dtype=torch.uint8, pin_memory=True) for _ in range(self.SLOTS if self._layout else 0)]
    self._events = [None] * self.SLOTS                       # upload of slot i finished (host may rewrite its staging block)
    self._host = [{k: st.numpy()[off:off + nb].view(dt).reshape(shape) for k, (off, nb, dt, shape) in self._layout.items()}
                  for st in self._stage]
    return self

  def view(self, key):
    """The device tensor of one entry (a view of the block: static address, graph-safe)."""
    import torch
    off, nb, dt, shape = self._layout[key]
    tdt = torch.from_numpy(np.empty(0, dt)).dtype
    return self.block[off:off + nb].view(tdt).view(shape)

  def has(self, key):
    return key in self._layout

  @property
  def is_open(self):
    return self._open

  def begin(self):
    i = self._turn % self.SLOTS
    if self._layout and self._events[i] is not None:
      self._events[i].synchronize()
    self._open = True

  def write(self, key, values):
    if not self._open:
      raise RuntimeError('FeedArena.write outside begin() / flush()')
    dst = self._host[self._turn % self.SLOTS][key]
    values = np.asarray(values)
    if values.shape != dst.shape:
      raise ValueError("feed '%s': expected shape %s, got %s" % (key[-1], dst.shape, values.shape))
    np.copyto(dst, values, casting='same_kind')

  def flush(self):
    import torch
    self._open = False
    if not self._layout:          # nothing is fed through the arena (e.g. every input is a device tensor): no copy to queue
      return
    i = self._turn % self.SLOTS
    self.block.copy_(self._stage[i], non_blocking=True)
    if self._events[i] is None:
      self._events[i] = torch.cuda.Event()
    self._events[i].record()
    self._turn += 1


class WindowFeed:
  """The static feed slot of one DeviceWindows feature (what the Estimator hands the model_fn in place of a dense tensor).

  The model picks ONE form (``form``) before its graph is captured; ``feed(windows)`` then repoints / refills per batch, and
  everything is stream-ordered in front of the replay.  The arena entries of every form the slot can take are reserved at
  construction, from the first batch:
    * 'pointers' (``pointers()``): an int64 device table of per-sample window addresses (an entry of the step's FeedArena); the
      model's input kernel reads the resident uint8 frames itself (ops.goal_dynimgs_u8_into), the fp32 windows are never written.
      Only offered when ``u8`` (every segment of the first batch is uint8 frames with divisor 255).
    * 'dense' (``dense()``): a float32 [n, K, *frame_shape] buffer filled by geeco_gather_windows, one launch per segment.
    * 'dense_by_address' (``dense()`` of a slot whose first batch came from a shuffling input, ``DeviceWindows.scattered``: about
      one segment per window): that buffer filled by ONE geeco_gather_windows_by_address launch that follows a window table riding
      in the arena.  The table reaches the device with the arena's copy, so ``after_flush()`` queues the launch, behind the flush.
    * 'dense_augmented' (``dense()`` of a slot whose first batch came from an augmenting input, ``DeviceWindows.augmented``):
      that buffer filled by ONE geeco_gather_windows_augmented launch; the window table, the batch's shifts and, for an RGB
      stream, its colour gains and biases ride in the arena, and ``after_flush()`` queues the launch as for 'dense_by_address'.
      Such a slot is never ``u8``: augmented windows exist only as dense windows.  An RGB stream whose draws carry scene extras
      (``DeviceWindows.scene_tables()``: occluders, sensor noise) is filled by ONE geeco_gather_windows_scene launch
      instead; the rectangles, their colours and the noise key ride in the arena too, sigma and the tag are launch arguments.
    * 'dense_frames' (``dense()`` of an augmented slot whose first batch carries frame sources, ``DeviceWindows.frame_src``: frame
      drops and camera lag): that buffer filled by ONE geeco_gather_windows_frames launch.  Its [n][K] table of
      frame addresses rides in the arena in place of the [n] window table, next to whichever of the tables above the draws
      carry: no copy and no launch more than 'dense_augmented'.  A batch without ``frame_src`` sends the consecutive table.
    * 'frame_table' (``frame_table()``, models built with shared_frames=F): the batch's distinct frames, see there.
  The three by-address forms queue their launch through ``device_windows._gather_by_tables``, which picks the entry point from
  the tables the slot reserved."""

  def __init__(self, windows, arena, key, shared_frames=None, shared_targets=None):
    """``shared_frames`` (a capacity F; the 'rgb' slot of a model built with shared_frames=F): the arena also carries the
    batch's frame table [F], frame index [n][K] and, with ``shared_targets`` (the key of the target stream in the same
    batch), target index [n] -- see ``frame_table``."""
    self.n, self.K, self.frame_shape, self.squeeze_k = windows.n, windows.K, windows.frame_shape, windows.squeeze_k
    self.arena, self.key, self.device = arena, key, arena.device
    self.scattered, self.augmented = bool(getattr(windows, 'scattered', False)), getattr(windows, 'augment', None) is not None
    self.u8 = windows.is_u8() and not self.augmented       # the slot can offer ``pointers()``
    self.shape = tuple(windows.shape)
    self.frames = getattr(windows, 'frame_src', None) is not None      # the slot follows one address per FRAME
    # 'pointers', 'dense', 'dense_by_address', 'dense_augmented', 'dense_frames' or 'frame_table' once the model chose
    self.form = None
    self.table = self.buffer = None
    # frame-table slots reserved in the arena (None: built without shared_frames) / in use (``frame_table()`` may take fewer)
    self.shared_reserved = self.shared = shared_frames
    self.shared_targets, self._with_targets = shared_targets, False
    self._gather_pending, self._window_tables = False, None
    scene = windows.scene_tables() if self.augmented else None
    # which extras an augmented RGB slot carries ('occlude', 'noise', 'occlude+noise'; None: the merged augmented fill)
    self.scene, self._scene_args = (windows.augment.scene if scene is not None else None), None
    if shared_frames is not None:
      arena.reserve(key + ('frame_table',), (int(shared_frames),), np.int64)
      arena.reserve(key + ('frame_index',), (self.n, self.K), np.int32)
      if shared_targets is not None:
        arena.reserve(key + ('target_index',), (self.n,), np.int32)
    # The batches whose frames a QUEUED replay may still read through the address table: the host runs up to
    # FeedArena.SLOTS feeds ahead of the device, so that many (+ the one being written) stay referenced here.  The uploads
    # of the prefetch thread and the replays share the default stream today (the caching allocator then orders any reuse
    # behind the replays anyway); this bound does not rely on that.
    self._live = collections.deque(maxlen=FeedArena.SLOTS + 1)
    if self.u8:
      arena.reserve(key, (self.n,), np.int64)
    if self.scattered or self.augmented:
      arena.reserve(key + ('window_addr',), (self.n, self.K) if self.frames else (self.n,), np.int64)
      arena.reserve(key + ('window_kind',), (self.n,), np.int32)
    if self.augmented:
      windows.augment_tables()                      # (raises on frames that are not [H, W, 3] / [H, W, 1])
      arena.reserve(key + ('aug_shift',), (self.n, 2), np.int32)
      if self.frame_shape[-1] == 3:
        arena.reserve(key + ('aug_colour',), (self.n, 6), np.float32)
      if scene is not None and scene[0] is not None:
        arena.reserve(key + ('aug_occ_rect',), (self.n, 4, 4), np.int32)
        arena.reserve(key + ('aug_occ_colour',), (self.n, 4, 3), np.float32)
      if scene is not None and scene[2] is not None:
        arena.reserve(key + ('aug_noise_key',), (2,), np.int32)

  adopted = property(lambda self: self.form is not None)      # the model took this slot as an input: it chose a form
  feeds_frame_table = property(lambda self: self.form == 'frame_table')

  def _choose(self, form):
    if self.form not in (None, form):
      raise RuntimeError("WindowFeed: the slot already feeds its '%s' form, '%s' asked for" % (self.form, form))
    self.form = form

  def pointers(self):
    if not self.u8:
      raise RuntimeError('WindowFeed.pointers(): the windows are not uint8 frames')
    self._choose('pointers')
    if self.arena.block is not None:
      self.table = self.arena.view(self.key)
    return self

  def frame_table(self, capacity=None, with_targets=True):
    """{'frame_table' [capacity], 'frame_index' [n][K][, 'target_index' [n]]} device views of the arena that ``feed`` rewrites
    per batch from ``DeviceWindows.frame_table``; neither fp32 windows nor per-window address tables are written.
    ``capacity`` <= the slots reserved at construction (default: all of them)."""
    if self.shared_reserved is None:
      raise RuntimeError('WindowFeed.frame_table(): the slot was built without shared_frames')
    capacity = self.shared_reserved if capacity is None else int(capacity)
    if capacity > self.shared_reserved:
      raise ValueError('WindowFeed.frame_table(): %d slots asked for, %d reserved' % (capacity, self.shared_reserved))
    if with_targets and self.shared_targets is None:
      raise RuntimeError('WindowFeed.frame_table(): the batch has no target stream')
    self._choose('frame_table')
    self.shared, self._with_targets = capacity, bool(with_targets)
    out = {'frame_table': self.arena.view(self.key + ('frame_table',))[:capacity],
           'frame_index': self.arena.view(self.key + ('frame_index',))}
    if with_targets:
      out['target_index'] = self.arena.view(self.key + ('target_index',))
    return out

  def dense(self):
    import torch
    self._choose('dense_frames' if self.frames else 'dense_augmented' if self.augmented else 'dense_by_address' if self.scattered else 'dense')
    if self.buffer is None:
      self.buffer = torch.empty(self.shape, dtype=torch.float32, device=self.device)
    return self.buffer

  def feed(self, windows, batch=None):
    """``batch``: the dict ``windows`` came from (the frame-table form looks its target stream up there).  A slot no model
    adopted feeds nothing."""
    if (windows.n, windows.K, windows.frame_shape) != (self.n, self.K, self.frame_shape):
      raise ValueError('WindowFeed: batch of %s windows does not fit the slot %s' % (tuple(windows.shape), self.shape))
    if (getattr(windows, 'augment', None) is not None) != self.augmented:
      raise RuntimeError('WindowFeed: %s windows in a slot built for %s ones (the Estimator keys its models by the batch being '
                         'augmented)' % (('plain', 'augmented') if self.augmented else ('augmented', 'plain')))
    self._gather_pending = False
    if self.form is not None:
      getattr(self, '_feed_' + self.form)(windows, batch)

  def _feed_pointers(self, windows, batch):
    if not windows.is_u8():
      raise RuntimeError('WindowFeed: float32 frames in a slot whose model reads uint8 frames (the Estimator keys its '
                         'models by the frame type)')
    self.arena.write(self.key, windows.addresses(self.device))
    self._live.append(windows)

  def _feed_dense(self, windows, batch):
    windows.materialize_into(self.buffer.view((self.n, self.K) + self.frame_shape))

  def _feed_dense_by_address(self, windows, batch):
    if getattr(windows, 'frame_src', None) is not None and not self.frames:
      raise RuntimeError('WindowFeed: a batch with frame sources in a slot built for consecutive windows (the Estimator keys its '
                         'models by them)')
    addr, kinds = windows.frame_addresses(self.device) if self.frames else windows.window_table(self.device)
    self.arena.write(self.key + ('window_addr',), addr)
    self.arena.write(self.key + ('window_kind',), kinds)
    self._live.append(windows)
    self._gather_pending = True       # the launch itself: after_flush()

  def _feed_dense_augmented(self, windows, batch):
    shift, colour = windows.augment_tables()
    self._feed_dense_by_address(windows, batch)
    self.arena.write(self.key + ('aug_shift',), shift)
    if colour is not None:
      self.arena.write(self.key + ('aug_colour',), colour)
    scene = windows.scene_tables()
    if (windows.augment.scene if scene is not None else None) != self.scene:
      raise RuntimeError('WindowFeed: a batch with the scene extras %r in a slot built for %r (the Estimator keys its models by '
                         'them)' % (windows.augment.scene if scene is not None else None, self.scene))
    if scene is not None:
      occ_rect, occ_colour, noise_key, sigma, tag = scene
      if occ_rect is not None:
        self.arena.write(self.key + ('aug_occ_rect',), occ_rect)
        self.arena.write(self.key + ('aug_occ_colour',), occ_colour)
      if noise_key is not None:
        self.arena.write(self.key + ('aug_noise_key',), noise_key)
      self._scene_args = (sigma, tag)

  _feed_dense_frames = _feed_dense_augmented      # the same tables; _feed_dense_by_address writes the [n][K] one

  def _feed_frame_table(self, windows, batch):
    targets = None
    if self._with_targets:
      targets = (batch or {}).get(self.shared_targets)
      if not isinstance(targets, DeviceWindows):
        raise RuntimeError("WindowFeed: the shared frame table needs the batch's '%s' as DeviceWindows" % self.shared_targets)
    table, index, tindex, _ = windows.frame_table(self.shared, targets, self.device)      # (raises on a mixed batch)
    if windows.is_u8() != self.u8:
      raise RuntimeError('WindowFeed: frames of another type than the slot was built for (the Estimator keys its models by the '
                         'frame type)')
    self.arena.write(self.key + ('frame_table',), np.pad(table, (0, self.shared_reserved - self.shared)))      # 0 = unused slot
    self.arena.write(self.key + ('frame_index',), index)
    if tindex is not None:
      self.arena.write(self.key + ('target_index',), tindex)
    self._live.append((windows, targets))

  def after_flush(self):
    """The by-address or augmented fill of the dense buffer, queued behind the arena's copy (which carries this batch's window
    table and augmentation draws) and in front of the replay.  Does nothing for the other forms."""
    if not self._gather_pending:
      return
    self._gather_pending = False
    if self._window_tables is None:       # static views of the sealed arena
      view = lambda name: self.arena.view(self.key + (name,)) if self.arena.has(self.key + (name,)) else None
      self._window_tables = tuple(view(name) for name in ('window_addr', 'window_kind', 'aug_shift', 'aug_colour', 'aug_occ_rect',
                                                          'aug_occ_colour', 'aug_noise_key'))
    sigma, tag = self._scene_args if self.scene is not None else (0.0, 0)
    _gather_by_tables(self.buffer, self._window_tables, sigma, tag, self.form == 'dense_frames', self.n, self.K, self.frame_shape)


# ---- the slots of one model (Estimator._get_spec) and the feed of one step ------------------------------------------------
class FeedDict(dict):
  """name -> static buffer (a view of the model's FeedArena, a WindowFeed, or a device tensor) of the features or the labels."""

  def __init__(self, arena, tag, items):
    super().__init__(items)
    self.arena, self.tag = arena, tag


def build_slots(device, feats, labels, shared_capacity=None):
  """(feature slots, label slots or None) for a model whose batches look like ``feats`` / ``labels``: ONE arena for everything
  the host writes per batch (states, labels, window address tables), sealed.  ``shared_capacity(K, goal)`` (models built with
  shared_frames): the slots of the frame table the 'rgb' WindowFeed reserves."""
  import torch
  arena = FeedArena(device)
  own = {}        # (tag, name) -> WindowFeed or device tensor; every other entry is a view of the arena
  for tag, d in (('features', feats), ('labels', labels)):
    for k, v in (d or {}).items():
      if isinstance(v, DeviceWindows):        # windows of HBM-resident episodes
        kw = {}
        if shared_capacity is not None and (tag, k) == ('features', 'rgb'):
          # room for the table either model_fn asks for (the goal model's holds the target frames too)
          has_tgt = isinstance(feats.get('target_rgb'), DeviceWindows)
          kw = dict(shared_frames=shared_capacity(v.K, has_tgt), shared_targets='target_rgb' if has_tgt else None)
        own[tag, k] = WindowFeed(v, arena, (tag, k), **kw)
      elif isinstance(v, np.ndarray) and v.nbytes <= ARENA_MAX_BYTES:
        arena.reserve((tag, k), v.shape, v.dtype)
      else:                                   # device tensors (synthetic inputs), dense host windows: a buffer and a copy of their own
        own[tag, k] = torch.as_tensor(v).to(device).contiguous()
  arena.seal()
  slots = lambda tag, d: None if d is None else FeedDict(
      arena, tag, {k: own[tag, k] if (tag, k) in own else arena.view((tag, k)) for k in d})
  return slots('features', feats), slots('labels', labels)


def adopted_slots(fbuf, lbuf, model_inputs):
  """Only the slots the model adopted are fed per batch: a WindowFeed whose form was chosen, a tensor or arena view that IS one
  of ``model_inputs``."""
  used = {id(v) for v in model_inputs.values()}
  keep = lambda bufs, tag: FeedDict(fbuf.arena, tag, {k: v for k, v in (bufs or {}).items()
                                                      if (v.adopted if isinstance(v, WindowFeed) else id(v) in used)})
  return keep(fbuf, 'features'), keep(lbuf, 'labels')


def _write(bufs, batch):
  """One dict of a batch into its slots, between the arena's ``begin`` and ``flush``."""
  import torch
  for k, buf in bufs.items():
    src = batch[k]
    if isinstance(buf, WindowFeed):          # repoint the address / frame tables or gather into the dense buffer
      buf.feed(src, batch)
    elif bufs.arena.has((bufs.tag, k)):
      bufs.arena.write((bufs.tag, k), src.detach().cpu().numpy() if torch.is_tensor(src) else src)
    elif isinstance(src, DeviceWindows):     # (a slot built from a dense first batch)
      src.materialize_into(buf.view((len(src), src.K) + src.frame_shape))
    else:
      buf.copy_(torch.as_tensor(src), non_blocking=True)


def feed_step(fbuf, lbuf, feats, labels):
  """Features and labels of one step: every host array through the arena's ONE staging block and copy; then what a slot queues
  BEHIND that copy and in front of the replay (WindowFeed.after_flush: the by-address fill of dense windows reads its window
  table from the arena on the device)."""
  fbuf.arena.begin()
  try:
    for bufs, batch in ((fbuf, feats), (lbuf, labels)):
      if bufs is not None and batch is not None:
        _write(bufs, batch)
  finally:
    fbuf.arena.flush()
  for bufs in (fbuf, lbuf):
    for buf in (bufs or {}).values():
      if isinstance(buf, WindowFeed):
        buf.after_flush()
