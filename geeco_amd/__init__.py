"""geeco_amd -- MI355X-native implementation of GEECO's e2evmc training hot path.

The compute path is the hand-written HIP library ``libgeeco_hip.so`` (geeco_amd/csrc, C ABI in
include/geeco_hip.h); the Python modules mirror the reference's call surface
(``params``, ``graph``, ``estimator``, ``input_fn``) on top of it.
"""
__version__ = '0.1.0'


def __getattr__(name):
  """``geeco_amd.EpisodeReplay`` (replay.py), ``geeco_amd.DynamicImageReplay`` and ``geeco_amd.open_replay`` (replay_dynimg.py),
  imported on first use: the package itself imports neither torch nor the library."""
  if name == 'EpisodeReplay':
    from .replay import EpisodeReplay
    return EpisodeReplay
  if name in ('DynamicImageReplay', 'open_replay'):
    from . import replay_dynimg
    return getattr(replay_dynimg, name)
  raise AttributeError('module %r has no attribute %r' % (__name__, name))
