"""TensorBoard event files without TensorFlow.

The reference logs every term of ``GraphKeys.LOSSES`` with ``tf.summary.scalar`` + ``SummarySaverHook``
(``src/models/e2evmc/estimator.py:305-313``) and the Estimator adds loss / global_step; TensorBoard then reads
``<model_dir>/events.out.tfevents.*``.  This writer produces such a file: TFRecord framing (u64 length, masked
CRC-32C of the length, payload, masked CRC-32C of the payload; uncompressed) around ``Event`` protos
  Event   { double wall_time = 1; int64 step = 2; string file_version = 3; Summary summary = 5; }
  Summary { repeated Value value = 1; }      Value { string tag = 1; float simple_value = 2; }
with the mandatory first record ``file_version = "brain.Event:2"``.

Histograms (params['variable_stats'] = 'histograms') are ``Value { string tag = 1; HistogramProto histo = 5; }`` with
  HistogramProto { double min = 1, max = 2, num = 3, sum = 4, sum_squares = 5; packed double bucket_limit = 6, bucket = 7; }
whose buckets are the magnitude classes of ``geeco_variable_stats``, listed by their ascending upper edges (``histogram_edges``): an
empty bucket with the edge -DBL_MAX, the negative classes from the largest magnitudes down (the class of exponent e, values in
(-2^(e+1), -2^e], has the upper edge -2^e), one bucket with the edge 0 for the zeros, and the positive classes (exponent e, values in
[2^e, 2^(e+1)), upper edge 2^(e+1)); the clamped outermost classes reach to -+DBL_MAX.  Non-finite elements are in no bucket.
"""
from __future__ import annotations

import os
import socket
import struct
import time

from ._native import VARSTATS_CLASSES as CLASSES
from .tfrecord import _enc_len, _enc_varint, masked_crc32c


# CLASSES = GEECO_VARSTATS_CLASSES of include/geeco_hip.h: class k holds 2^(k-32) <= |x| < 2^(k-31), clamped at both ends
_DBL_MAX = 1.7976931348623157e308


def histogram_edges():
  """The ascending upper edges of the 2 * CLASSES + 2 buckets: an empty one that ends at -DBL_MAX (the lower edge of the clamped negative
  class 39), the negative classes from the largest magnitude down, the zeros, the positive classes."""
  neg = [-(2.0 ** (k - 32)) for k in range(CLASSES - 1, -1, -1)]      # class 39 first: its upper edge is -2^7
  pos = [2.0 ** (k - 31) for k in range(CLASSES - 1)] + [_DBL_MAX]
  return [-_DBL_MAX] + neg + [0.0] + pos


def histogram_proto(h):
  """``h``: dict(min, max, num, sum, sum_squares, zeros, neg[CLASSES], pos[CLASSES]) -> HistogramProto bytes."""
  buckets = [0.0] + [float(x) for x in reversed(h['neg'])] + [float(h['zeros'])] + [float(x) for x in h['pos']]
  out = b''
  for field, key in ((1, 'min'), (2, 'max'), (3, 'num'), (4, 'sum'), (5, 'sum_squares')):
    out += _enc_varint((field << 3) | 1) + struct.pack('<d', float(h[key]))
  out += _enc_len(6, b''.join(struct.pack('<d', e) for e in histogram_edges()))
  out += _enc_len(7, b''.join(struct.pack('<d', b) for b in buckets))
  return out


def _histogram_event(wall_time, step, histograms):
  out = _enc_varint((1 << 3) | 1) + struct.pack('<d', float(wall_time)) + _enc_varint((2 << 3) | 0) + _enc_varint(int(step))
  summary = b''
  for tag, h in histograms.items():
    summary += _enc_len(1, _enc_len(1, tag.encode()) + _enc_len(5, histogram_proto(h)))
  return out + _enc_len(5, summary)


def _event(wall_time, step=None, file_version=None, scalars=None):
  out = _enc_varint((1 << 3) | 1) + struct.pack('<d', float(wall_time))
  if step is not None:
    out += _enc_varint((2 << 3) | 0) + _enc_varint(int(step))
  if file_version is not None:
    out += _enc_len(3, file_version.encode())
  if scalars:
    summary = b''
    for tag, value in scalars.items():
      v = _enc_len(1, tag.encode()) + _enc_varint((2 << 3) | 5) + struct.pack('<f', float(value))
      summary += _enc_len(1, v)
    out += _enc_len(5, summary)
  return out


class EventFileWriter:
  """Appends scalar summaries to ``<logdir>/events.out.tfevents.<time>.<host>``."""

  def __init__(self, logdir):
    os.makedirs(logdir, exist_ok=True)
    self.path = os.path.join(logdir, 'events.out.tfevents.%010d.%s' % (int(time.time()), socket.gethostname()))
    self._f = open(self.path, 'ab')
    self._write(_event(time.time(), file_version='brain.Event:2'))

  def _write(self, payload):
    hdr = struct.pack('<Q', len(payload))
    self._f.write(hdr + struct.pack('<I', masked_crc32c(hdr)) + payload + struct.pack('<I', masked_crc32c(payload)))
    self._f.flush()

  def add_scalars(self, scalars: dict, step: int, wall_time=None):
    self._write(_event(time.time() if wall_time is None else wall_time, step=step, scalars=scalars))

  def add_histograms(self, histograms: dict, step: int, wall_time=None):
    """``histograms``: {tag: what ``histogram_proto`` takes}; one event record."""
    self._write(_histogram_event(time.time() if wall_time is None else wall_time, step, histograms))

  def close(self):
    self._f.close()
