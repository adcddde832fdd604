"""Fake resident episodes and a recording arena for the host-side tests of DeviceWindows and WindowFeed (no GPU)."""
import numpy as np
import torch

from geeco_amd.device_windows import DeviceWindows

SHAPE = (4, 6, 3)
FE = int(np.prod(SHAPE))
K = 3


class FakeFrames:
  """Stands in for an episode's resident frame tensor [T, frame_elems]: an address, a length, a dtype, a device."""

  def __init__(self, base, T, dtype=torch.uint8, device='cuda:0'):
    self.base, self.shape, self.dtype, self.device = base, (T, FE), dtype, torch.device(device)

  def data_ptr(self):
    return self.base

  def is_contiguous(self):
    return True


def windows(segments, k=K, squeeze=False):
  dw = DeviceWindows(k, SHAPE, 255.0, squeeze_k=squeeze)
  for frames, starts, div in segments:
    dw.add(frames, np.asarray(starts, np.int32), div)
  return dw


class RecordingArena:
  """The FeedArena calls WindowFeed makes, on the host, with a log of their order."""

  def __init__(self, log):
    self.device, self.log, self.layout, self.values, self.block = torch.device('cpu'), log, {}, {}, None

  def reserve(self, key, shape, dtype):
    self.layout[key] = (tuple(shape), np.dtype(dtype))

  def has(self, key):
    return key in self.layout

  def seal(self):
    self.block = True

  def write(self, key, values):
    shape, dt = self.layout[key]
    assert np.asarray(values).shape == shape and np.asarray(values).dtype == dt, key
    self.values[key] = np.array(values)
    self.log.append(('write', key[-1]))

  def view(self, key):
    return ('view',) + key

  def flush(self):
    self.log.append(('flush',))
