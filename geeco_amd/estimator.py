"""Estimator-style training harness and the two ``model_fn``s.

Mirrors the call surface that the reference's ``scripts/train_e2evmc.py:210-291`` touches:
``Estimator(model_fn=, model_dir=, config=, params=)``, ``.train(input_fn=)``,
``.evaluate(input_fn=) -> {'loss', 'cmd_ee', 'pos_ee', 'pos_obj', 'cmd_grp', 'global_step'}``,
``RunConfig``, ``GPUOptions`` / ``ConfigProto``, ``ModeKeys``, ``EstimatorSpec``,
``latest_checkpoint`` -- and ``e2evmc_model_fn`` / ``goal_e2evmc_model_fn`` with the signature
``model_fn(features, labels, mode, params)`` of ``src/models/e2evmc/estimator.py:14,144``.

Graph-mode semantics are kept: ``model_fn`` is called ONCE per (mode, batch size) with the static
device buffers that will hold every batch; it builds the model on the HIP kernels and returns an
``EstimatorSpec`` whose ``train_op`` replays the captured step.  The Estimator's loop then only
copies each batch into those buffers and calls ``train_op()``  (= ``session.run(train_op)``).
State lives in ``model_dir`` as ``model.ckpt-<step>.pt`` + a TF-style ``checkpoint`` index file.
"""
from __future__ import annotations

import collections
import collections.abc
import json
import math
import os
import re
import time

import torch

from . import dist as gdist
from . import feed
from . import graph
from .device_windows import DeviceWindows
from .runtime import EvalStepRunner, TrainStepRunner, dp_form_kwargs
from .tf_checkpoint import EMA_SUFFIX
from .train_options import PARAMS, TrainOptions, check_exclusions
from .variables import model_variable_shapes


class ModeKeys:
  TRAIN = 'train'
  EVAL = 'eval'
  PREDICT = 'infer'


class GPUOptions:
  """tf.GPUOptions(allow_growth, per_process_gpu_memory_fraction) (train_e2evmc.py:217-219)."""

  def __init__(self, allow_growth=True, per_process_gpu_memory_fraction=None):
    self.allow_growth = allow_growth
    self.per_process_gpu_memory_fraction = per_process_gpu_memory_fraction


class ConfigProto:

  def __init__(self, gpu_options=None):
    self.gpu_options = gpu_options or GPUOptions()


class RunConfig:
  """tf.estimator.RunConfig(session_config, save_checkpoints_steps, keep_checkpoint_max) (train_e2evmc.py:221-224)."""

  def __init__(self, session_config=None, save_checkpoints_steps=None, keep_checkpoint_max=5, device=None,
               use_hipgraph=True, init_seed=0, save_tf_bundle=False, dp_form=None):
    self.session_config = session_config or ConfigProto()
    self.save_checkpoints_steps = save_checkpoints_steps
    self.keep_checkpoint_max = keep_checkpoint_max
    self.device = device
    self.use_hipgraph = use_hipgraph
    self.init_seed = init_seed
    # also write every checkpoint as a TF-1.15 tensor bundle (model.ckpt-<step>.index / .data-00000-of-00001 with the
    # reference's variable names, Adam slots and global_step): what tf.train.Saver consumers such as the reference's
    # predictor (predictor.py:85-95) and _export_snapshot (train_e2evmc.py:160-181) expect to find
    self.save_tf_bundle = save_tf_bundle
    # data parallel only: the form of the step (runtime.DP_FORMS).  None = 'three_graphs_reserve16' -- every
    # collective an ordinary RCCL launch between three replayed graphs (safe with ragged epochs by construction), part 2's persistent
    # kernels leaving 16 CUs to RCCL's workgroups, which cannot share a CU with them (profiles/HARDWARE_FINDINGS.md 37).  'overlap'
    # (the whole step incl. both all-reduces as ONE hipGraph), 'overlap_reserve16/32', 'serial', 'three_graphs_serial' are
    # opt-in: take the one bench.py reports as fastest on the node at hand (comm.step_ms / comm.timed_form of an N > 1 run)
    self.dp_form = dp_form


EstimatorSpec = collections.namedtuple(
    'EstimatorSpec', ['mode', 'loss', 'train_op', 'eval_metric_ops', 'predictions', 'training_hooks',
                      'evaluation_hooks', 'model'])
EstimatorSpec.__new__.__defaults__ = (None,) * 7


# ================================================================================================
# checkpoints (TF-style names so that _export_snapshot-like tooling works unchanged)
# ================================================================================================
_BUNDLE_SUFFIXES = ('.index', '.data-00000-of-00001')


def latest_checkpoint(model_dir):
  """tf.train.latest_checkpoint: '<model_dir>/model.ckpt-<step>' or None (train_e2evmc.py:160).  The prefix counts
  when its native file (.pt) or its TF tensor bundle (.index) exists."""
  index = os.path.join(model_dir, 'checkpoint')
  if not os.path.exists(index):
    return None
  with open(index) as f:
    m = re.search(r'model_checkpoint_path:\s*"([^"]+)"', f.read())
  if not m:
    return None
  path = os.path.join(model_dir, os.path.basename(m.group(1)))
  return path if (os.path.exists(path + '.pt') or os.path.exists(path + '.index')) else None


def save_checkpoint(store, model_dir, keep_max, tf_bundle=False, lstm_batch=None):
  step = int(store.global_step.item())
  name = 'model.ckpt-%d' % step
  tmp = os.path.join(model_dir, name + '.pt.tmp')
  torch.save(store.state_dict(), tmp)
  os.replace(tmp, os.path.join(model_dir, name + '.pt'))
  if tf_bundle:
    from . import tf_checkpoint
    mem = [n.rsplit('/', 2)[0] + '/lstm_memory' for n in store.shapes if n.endswith('/lstm_cell/kernel')]
    tf_checkpoint.export_checkpoint(store, os.path.join(model_dir, name), lstm_memory_name=mem[0] if mem else None,
                                    batch_size=lstm_batch)
  existing = sorted((int(re.match(r'model\.ckpt-(\d+)\.pt$', fn).group(1)) for fn in os.listdir(model_dir)
                     if re.match(r'model\.ckpt-(\d+)\.pt$', fn)))
  if keep_max and len(existing) > keep_max:
    for s in existing[:-keep_max]:
      for suffix in ('.pt',) + _BUNDLE_SUFFIXES:
        fn = os.path.join(model_dir, 'model.ckpt-%d%s' % (s, suffix))
        if os.path.exists(fn):
          os.remove(fn)
    existing = existing[-keep_max:]
  with open(os.path.join(model_dir, 'checkpoint'), 'w') as f:
    f.write('model_checkpoint_path: "%s"\n' % name)
    for s in existing:
      f.write('all_model_checkpoint_paths: "model.ckpt-%d"\n' % s)
  return os.path.join(model_dir, name)


def load_checkpoint(store, prefix):
  """Native .pt file when present, else the TF-1.15 tensor bundle of the same prefix (parameters, Adam slots, step)."""
  if os.path.exists(prefix + '.pt'):
    store.load_state_dict(torch.load(prefix + '.pt', map_location='cpu'))
  else:
    from . import tf_checkpoint
    tf_checkpoint.import_checkpoint(store, prefix, load_optimizer=True)


def check_warm_start(value, key='warm_start_from'):
  """``warm_start_from`` normalised (the counterpart of tf.estimator.WarmStartSettings): None = off; a path (a model_dir or a checkpoint
  prefix), or a mapping with 'ckpt' (such a path), 'vars' (a regular expression ``re.search``es in the NEW model's variable names:
  which ones to warm-start; default '.*') and 'name_map' ({prefix of the new name: prefix in the checkpoint}, the first that the
  name starts with is applied).  Returns dict(ckpt=, vars=, name_map=) or None; anything else raises ValueError naming ``key``."""
  if value is None or value == '':
    return None
  if isinstance(value, (str, os.PathLike)):
    value = {'ckpt': value}
  if not isinstance(value, collections.abc.Mapping) or not isinstance(value.get('ckpt'), (str, os.PathLike)) or not value.get('ckpt'):
    raise ValueError("%s=%r: a path, or a mapping with 'ckpt' (a model_dir or a checkpoint prefix), 'vars' and 'name_map'" % (key, value))
  for field in value:
    if field not in ('ckpt', 'vars', 'name_map'):
      raise ValueError("%s: unknown field %r (known: ckpt, vars, name_map)" % (key, field))
  pattern = value.get('vars', '.*')
  pattern = '.*' if pattern is None else pattern
  try:
    re.compile(pattern)
  except (re.error, TypeError) as e:
    raise ValueError('%s: vars=%r is not a regular expression: %s' % (key, pattern, e))
  name_map = value.get('name_map') or {}
  if not isinstance(name_map, collections.abc.Mapping) or not all(isinstance(k, str) and isinstance(v, str) for k, v in name_map.items()):
    raise ValueError('%s: name_map=%r must map prefixes of the new names to prefixes in the checkpoint' % (key, name_map))
  return {'ckpt': os.fspath(value['ckpt']), 'vars': pattern, 'name_map': collections.OrderedDict(name_map)}


def _checkpoint_prefix(path):
  """A checkpoint prefix from a prefix or a model_dir (its latest checkpoint)."""
  if os.path.isdir(path):
    prefix = latest_checkpoint(path)
    if prefix is None:
      raise FileNotFoundError('warm_start_from: no checkpoint in %s' % path)
    return prefix
  for suffix in ('.pt', '.index'):
    if path.endswith(suffix):
      path = path[:-len(suffix)]
  if not (os.path.exists(path + '.pt') or os.path.exists(path + '.index')):
    raise FileNotFoundError('warm_start_from: neither %s.pt nor %s.index exists' % (path, path))
  return path


def warm_start(store, settings):
  """Starts ``store`` from somebody else's checkpoint (tf.estimator.WarmStartSettings).  ``settings``: what
  ``check_warm_start`` takes.  Every variable whose name matches 'vars' is read from the checkpoint -- the native .pt file when
  present, else the TF-1.15 bundle of the prefix -- under its name with the first matching 'name_map' prefix rewritten; everything
  else keeps the value it has (its fresh initialisation).  Parameters only: the Adam moments are zeroed, the step counter is 0, the
  averaged weights restart from the parameters.  KeyError naming a selected variable the checkpoint lacks, ValueError naming the
  variable and both shapes where they differ; the store is not touched then.  Returns the names that were warm-started."""
  import numpy as np
  st = check_warm_start(settings)
  prefix = _checkpoint_prefix(st['ckpt'])
  rx = re.compile(st['vars'])
  source = collections.OrderedDict()
  for name in store.shapes:
    if rx.search(name):
      old = name
      for new_prefix, old_prefix in st['name_map'].items():
        if name.startswith(new_prefix):
          old = old_prefix + name[len(new_prefix):]
          break
      source[name] = old
  if os.path.exists(prefix + '.pt'):
    sd = torch.load(prefix + '.pt', map_location='cpu')
    have = {}
    for n, shp, off in zip(sd['names'], sd['shapes'], sd['offsets']):
      if n in set(source.values()):
        have[n] = sd['params'][off:off + int(np.prod(shp))].reshape(tuple(shp)).numpy()
  else:
    from . import tf_checkpoint
    have = tf_checkpoint.read_checkpoint(prefix, names=set(source.values()))
  for name, old in source.items():
    if old not in have:
      raise KeyError('%s: warm start selects it, but checkpoint %s holds no variable %s' % (name, prefix, old))
    if tuple(have[old].shape) != tuple(store.shapes[name]):
      raise ValueError('%s: checkpoint %s holds %s with shape %s, the model needs %s'
                       % (name, prefix, old, tuple(have[old].shape), tuple(store.shapes[name])))
  for name, old in source.items():
    store.var(name).copy_(torch.from_numpy(np.ascontiguousarray(have[old], dtype=np.float32)))
  store.adam_m.zero_()
  store.adam_v.zero_()
  store.global_step.zero_()
  store._params_rewritten()
  return list(source)


def restore_for_inference(store, model_dir, checkpoint_name=None, use_ema=False):
  """The predictors' restore (predictor.py:85-95): the named checkpoint, else the latest one of the directory -- a native
  .pt file, or a TensorFlow-1.15 tensor bundle (e.g. the published geeco_models_icra21 weights).  Parameters only.
  ``use_ema``: the parameters are the checkpoint's averaged weights (params['ema_decay'] of the training run); KeyError naming the
  first missing tensor if it holds none."""
  ckpt = os.path.join(model_dir, checkpoint_name) if checkpoint_name else latest_checkpoint(model_dir)
  if ckpt is None:
    raise FileNotFoundError('no checkpoint in %s' % model_dir)
  if os.path.exists(ckpt + '.pt') and use_ema:
    sd = torch.load(ckpt + '.pt', map_location='cpu')
    if sd.get('ema') is None:
      raise KeyError('%s%s: checkpoint %s.pt holds no averaged weights' % (list(sd['names'])[0], EMA_SUFFIX, ckpt))
    store.load_state_dict(dict(sd, params=sd['ema']))
  elif os.path.exists(ckpt + '.pt'):
    load_checkpoint(store, ckpt)
  else:
    from . import tf_checkpoint
    tf_checkpoint.import_checkpoint(store, ckpt, load_optimizer=False, use_ema=use_ema)
  print('>>> Restored model parameters from %s%s' % (ckpt, ' (averaged weights)' if use_ema else ''))


# ================================================================================================
# model_fn (estimator.py:14-141 and 144-279)
# ================================================================================================
class _SummarySaverHook:
  """Counterpart of the per-loss-term SummarySaverHooks (estimator.py:305-313): every ``log_steps`` steps the loss
  terms go to a TensorBoard event file (<model_dir>/events.out.tfevents.*, tags ``loss`` and ``loss_<term>`` like the
  reference's tf.summary.scalar names) and as one JSON line to <model_dir>/events.jsonl."""

  _writers = {}     # one event file per model_dir and process

  def __init__(self, model, every):
    self.model, self.every = model, max(int(every), 1)

  @classmethod
  def _writer(cls, model_dir):
    if model_dir not in cls._writers:
      from .summary import EventFileWriter
      cls._writers[model_dir] = EventFileWriter(model_dir)
    return cls._writers[model_dir]

  def after_run(self, step, model_dir):
    if step % self.every:
      return
    if gdist.rank() != 0 and getattr(self.model, 'guard', None) is None:
      return
    self.model.check_device_errors()        # (the loss read-out below waits for the device anyway)
    # params['skip_nonfinite']: the limit is checked on EVERY rank -- the replicas decide alike, so all of them stop together
    skipped = check_skipped_steps(self.model)
    if gdist.rank() != 0:
      return
    parts = {k: float(v) for k, v in self.model.loss_parts().items()}
    stats = self.model.variable_stats() if getattr(self.model, 'stats_plan', None) is not None else None      # params['variable_stats']
    if getattr(self.model, 'clip_out', None) is not None:      # params['clip_norm'] / ['skip_nonfinite']: the norm of this step's gradient before clipping
      parts['grad_norm'] = float(self.model.clip_out[1])
    if getattr(self.model, 'guard', None) is not None:         # params['skip_nonfinite']: steps this model has skipped so far (not checkpointed)
      parts['skipped_steps'] = skipped
    if getattr(self.model, 'lr_schedule', None) is not None:   # params['lr_schedule']: the rate this step was taken with, as the device formed it
      parts['learning_rate'] = float(self.model.scal[2])
    parts['global_step'] = step
    parts['wall_time'] = time.time()
    scalars = {k: v for k, v in parts.items() if k.startswith('loss') or k == 'learning_rate'}
    histograms = {}
    if stats is not None:
      # params['variable_stats']: the scalars per variable, and on a step that was skipped the variables whose gradient was not finite
      # (a float that is not finite -- a sum of squares beyond float32 -- goes in as the string 'inf' / '-inf' / 'nan': strict JSON)
      parts['variables'] = {n: {k: (v if not isinstance(v, float) or math.isfinite(v) else str(v)) for k, v in d.items() if k != 'histograms'}
                            for n, d in stats.items()}
      if getattr(self.model, 'guard', None) is not None and not int(self.model.guard[0]):
        parts['nonfinite_variables'] = self.model.nonfinite_gradient_variables(stats)
      for n, d in stats.items():
        for key in ('grad_norm', 'weight_norm', 'update_ratio', 'grad_zero_fraction'):
          if d[key] is not None:
            scalars['%s/%s' % (key, n)] = d[key]
        for kind, h in d.get('histograms', {}).items():
          histograms['%s/%s' % (kind, n)] = h
    if model_dir:
      with open(os.path.join(model_dir, 'events.jsonl'), 'a') as f:
        f.write(json.dumps(parts) + '\n')
      self._writer(model_dir).add_scalars(scalars, step, parts['wall_time'])
      if histograms:
        self._writer(model_dir).add_histograms(histograms, step, parts['wall_time'])
    print('INFO: loss = %.6f, step = %d' % (parts['loss'], step), flush=True)


def check_skipped_steps(model):
  """params['skip_nonfinite']: the steps ``model`` has skipped in all (0 for a model without the option).  Raises
  RuntimeError once as many in a row as the limit were skipped: the input, not one batch, is broken.  READS the device: called
  where the host synchronises anyway."""
  if getattr(model, 'guard', None) is None:
    return 0
  _, total, row = (int(x) for x in model.guard.tolist())
  if row >= model.skip_limit:
    where = ''
    if getattr(model, 'stats_plan', None) is not None:      # params['variable_stats']: which variables held the non-finite elements
      bad = model.nonfinite_gradient_variables()
      where = '; non-finite gradient elements of the last skipped step: ' + (', '.join('%s: %d' % kv for kv in bad.items()) or 'none '
                                                                            '(the squares overflowed float32)')
    raise RuntimeError('geeco_amd: the last %d optimiser steps in a row were skipped for a non-finite gradient (%d skipped in all; norm of the '
                       "last one: %r; params['skip_nonfinite'] allows fewer than %d in a row); nothing was saved%s"
                       % (row, total, float(model.clip_out[1]), model.skip_limit, where))
  return total


def shared_frames_capacity(shared, N, K, goal):
  """Slots of the frame table for ``params['shared_frames']``: an integer is taken as given; True = N + 2 (K - 1), + 2 for the
  goal model.  N consecutive windows of ONE episode hold N + K - 1 distinct frames; input_fn shuffles episodes, not windows, so
  a batch no larger than the windows of an episode spans at most two episodes: N + 2 (K - 1) frames, and for the goal model one
  target frame per episode (the episode's last frame is uploaded beside the windowable ones).  A batch that needs more (batches
  larger than an episode's windows) makes the feed raise with the number needed: pass that as an integer."""
  if isinstance(shared, bool):
    return N + 2 * (K - 1) + (2 if goal else 0)
  return int(shared)


def _model_fn(features, labels, mode, params, goal):
  cfg = params['e2evmc_config']
  if cfg.img_channels not in (3, 4):
    raise ValueError("Unsupported number of channels for input frame: %d!" % cfg.img_channels)
  if mode not in (ModeKeys.TRAIN, ModeKeys.EVAL, ModeKeys.PREDICT):
    raise RuntimeError("Unknown estimator mode: %s" % (mode,))
  rgb = features['rgb']
  if rgb.device.type != 'cuda':
    raise RuntimeError('geeco_amd needs a GPU: model_fn got features on %s (no CPU fallback)' % rgb.device)
  N = int(rgb.shape[0])
  training = mode == ModeKeys.TRAIN
  ctor = graph.GoalE2EVMC if goal else graph.E2EVMC
  # the options of params, checked once; what the model of this mode takes of them; what they do not go with (train_options.py)
  checked = TrainOptions.from_params(params, cfg, model_variable_shapes(cfg, goal))
  opts = checked.for_mode(mode)
  shared = params.get('shared_frames')
  check_exclusions(opts, gdist.world_size(), shared_frames=shared, key=PARAMS)
  # params['ema_decay']: the store carries the shadow arena, the training step keeps it, and every other mode's model
  # is built on the store's shadow view -- its parameters ARE the averaged weights (an inference stack re-derives its weight
  # copies from them on every forward)
  store = params.get('_variable_store')
  if checked.ema_decay is not None:
    store = store or graph.build_store(cfg, goal, rgb.device, ema=True)
    if not training:
      store = store.shadow_view()
  tables = {}
  if shared:
    # params['shared_frames'] (True, or a capacity F): encode each distinct frame of the batch once
    if getattr(rgb, 'shared', None) is None:
      raise ValueError("params['shared_frames'] needs the windows as DeviceWindows (pickplace_input_fn(device='cuda')): "
                       "dense 'rgb' tensors hold every frame K times and no frame addresses")
    F = shared_frames_capacity(shared, N, cfg.window_size, goal)
    model = ctor(cfg, N, rgb.device, training=training, store=store, shared_frames=F, options=opts)
    tables = rgb.frame_table(F, with_targets=goal)
    model.frames_u8 = rgb.u8
    for k, v in tables.items():
      model.inputs[k] = v
  else:
    model = ctor(cfg, N, rgb.device, training=training, store=store, options=opts)
  # adopt the caller's static buffers as the model inputs (placeholders)
  source = lambda k: labels.get(k) if (labels is not None and k in model.label_keys) else features.get(k)
  # all of the model's image inputs that CAN come as window addresses must, or none does
  take_u8 = bool(model.u8_window_keys) and all(getattr(source(k), 'u8', False) for k in model.u8_window_keys)
  for k in list(model.inputs.keys()):
    if k in tables:
      continue
    src = source(k)
    if src is None:
      if mode == ModeKeys.PREDICT and k in model.label_keys + ['ee_state', 'obj_state']:
        continue   # label-side inputs are not needed for predictions
      raise KeyError("model_fn: missing input '%s'" % k)
    if hasattr(src, 'pointers'):
      # feed.WindowFeed, or the predictors' stand-in (windows of HBM-resident episodes): a model whose input kernel follows window addresses takes the
      # address table and the fp32 windows are never written; any other model gets the dense buffer the gather fills
      if tuple(src.shape) != tuple(model.inputs[k].shape):
        raise ValueError("model_fn: input '%s' must have shape %s, got %s" % (k, tuple(model.inputs[k].shape), tuple(src.shape)))
      if take_u8 and k in model.u8_window_keys:
        src.pointers()
        model.inputs[k] = src
      else:
        model.inputs[k] = src.dense()
    elif (src.is_cuda and src.dtype == torch.float32 and src.is_contiguous() and
        tuple(src.shape) == tuple(model.inputs[k].shape)):
      model.inputs[k] = src
    else:
      raise ValueError("model_fn: input '%s' must be a contiguous float32 device tensor of shape %s" %
                       (k, tuple(model.inputs[k].shape)))
  model._bind_labels()
  # the reference computes `reset` from features['step'] (estimator.py:41-42); it is numerically
  # inert (both tf.cond branches are zeros, graph.py:218-220), so it is validated and dropped.
  if 'step' in features and features['step'].dtype != torch.int64:
    raise ValueError("features['step'] must be int64")
  print('>>> Graph Summary (%d trainable parameters):' % (model.store.count_parameters(),))
  if mode == ModeKeys.TRAIN:
    runner = TrainStepRunner(model, use_graph=params.get('use_hipgraph', True), **dp_form_kwargs(params.get('dp_form')))
    hooks = [_SummarySaverHook(model, params.get('log_steps', 1000))]
    return EstimatorSpec(mode=mode, loss=model.loss, train_op=runner.step, training_hooks=hooks, model=model)
  runner = EvalStepRunner(model, use_graph=params.get('use_hipgraph', True))
  if mode == ModeKeys.EVAL:
    return EstimatorSpec(mode=mode, loss=model.loss, train_op=runner.step, eval_metric_ops=_eval_metric_fn(model),
                         evaluation_hooks=[], model=model)
  return EstimatorSpec(mode=mode, predictions=model.predictions(), train_op=runner.step, model=model)


def e2evmc_model_fn(features, labels, mode, params):
  """Unconditional reflex (scope 'VMC'); reference estimator.py:14-141."""
  return _model_fn(features, labels, mode, params, goal=False)


def goal_e2evmc_model_fn(features, labels, mode, params):
  """Goal-conditioned controller (scope 'GoalVMC'); reference estimator.py:144-279."""
  return _model_fn(features, labels, mode, params, goal=True)


def _eval_metric_fn(model):
  """Per-batch sufficient statistics for tf.metrics.mean_squared_error / accuracy
  (estimator.py:246-254): returns a callable giving {key: (sum, count)} device tensors."""
  K = model.K

  def batch_stats():
    p = model.predictions()
    inp = model.inputs
    tgt = {'pos_ee': inp['ee_state'][:, K - 1, :3], 'pos_obj': inp['obj_state'][:, K - 1, :3]}
    if model.cfg.control_mode == 'cartesian':
      tgt['cmd_ee'] = inp['cmd'][:, :3]
    else:                                                     # estimator.py:117-120 / 255-258
      tgt.update({'cmd_vel': inp['vel_target'], 'cmd_ee': inp['ee_target'][:, :3], 'cmd_grp': inp['grp_target']})
    out = {}
    for k, t in tgt.items():
      out[k] = (((p[k] - t) ** 2).sum(), float(t.numel()))
    if model.cfg.control_mode == 'cartesian':
      label = torch.round(inp['cmd'][:, 3]).to(torch.int64) + 1
      out['cmd_grp'] = ((p['logits_cmd_grp'].argmax(dim=-1) == label).float().sum(), float(label.numel()))
    return out
  return batch_stats


# ================================================================================================
# Estimator
# ================================================================================================
def _host_results(model, res, scalars=()):
  """What a pass of ``Estimator._input_pass`` yields for ``res``, its device results: one synchronisation, the device-error check, then
  every tensor as a numpy copy and the ones named in ``scalars`` as floats (entries that are no tensors are left out)."""
  torch.cuda.synchronize()
  model.check_device_errors()
  out = {k: v.detach().cpu().numpy().copy() for k, v in res.items() if torch.is_tensor(v) and k not in scalars}
  out.update({k: float(res[k]) for k in scalars if k in res})
  return out


class Estimator:
  """tf.estimator.Estimator counterpart (train_e2evmc.py:260-264, 284-291)."""

  def __init__(self, model_fn, model_dir=None, config=None, params=None, warm_start_from=None):
    """``warm_start_from`` (or params['warm_start_from']): ``check_warm_start``; applies only while ``model_dir`` holds no checkpoint
    of its own (``warm_start``)."""
    self._model_fn = model_fn
    self.model_dir = model_dir
    self.config = config or RunConfig()
    self.params = dict(params or {})
    # the options are checked here, as far as they can be before the model is known, so that a bad value raises at construction;
    # train() reads this record: ``params`` is final once the Estimator is built
    self.options = TrainOptions.from_params(self.params, self.params.get('e2evmc_config'), None)
    if warm_start_from is None:
      warm_start_from = self.params.get('warm_start_from')
    self.warm_start_from = check_warm_start(warm_start_from, "params['warm_start_from']" if 'warm_start_from' in self.params else 'warm_start_from')
    self._specs = {}          # (mode, N) -> (spec, feature buffers, label buffers)
    self.last_train_stats = None
    self._store = None
    self._restored = False
    self._finetune_logged = False
    self._loss_shaping_logged = False
    if model_dir and gdist.rank() == 0:
      os.makedirs(model_dir, exist_ok=True)
    frac = getattr(self.config.session_config.gpu_options, 'per_process_gpu_memory_fraction', None)
    if frac and torch.cuda.is_available() and 0.0 < frac < 1.0:
      torch.cuda.set_per_process_memory_fraction(float(frac))   # --memcap (train_e2evmc.py:102-104)

  # -- device / batches ------------------------------------------------------------------------
  def _device(self):
    if self.config.device is not None:
      return torch.device(self.config.device)
    if not torch.cuda.is_available():
      raise RuntimeError('geeco_amd.Estimator needs an MI355X (torch.cuda.is_available() is False); '
                         'there is no CPU fallback')
    return torch.device('cuda', torch.cuda.current_device())

  @staticmethod
  def _shard(batch, world, rank):
    """Slice of a GLOBAL batch for this rank (synthetic inputs / unsharded input_fns): contiguous, sizes differing by
    at most one, so a ragged global batch is kept (geeco_gym.py:471 has no drop_remainder).  Returns
    (features, labels, n_local, n_global); n_local may be 0."""
    feats, labels = batch
    n = int(feats['step'].shape[0]) if 'step' in feats else int(next(iter(feats.values())).shape[0])
    if world == 1:
      return feats, labels, n, n
    base, extra = divmod(n, world)
    lo = rank * base + min(rank, extra)
    hi = lo + base + (1 if rank < extra else 0)
    if hi == lo:
      return None, None, 0, n
    sl = lambda d: {k: v[lo:hi] for k, v in d.items()} if d is not None else None
    return sl(feats), sl(labels), hi - lo, n

  def _local_batches(self, it, world, rank):
    """Yields (features, labels, n_local, n_global) per optimiser step.  An input_fn that already sharded the
    episodes over the ranks (pickplace_input_fn(shard=...)) carries ``dp_schedule`` = every rank's window count per
    step; otherwise each rank slices the same global batch."""
    sched = getattr(it, 'dp_schedule', None) if world > 1 else None
    if sched is None:
      for batch in it:
        yield self._shard(batch, world, rank)
      return
    src = iter(it)
    for counts in sched:
      if counts[rank] > 0:
        feats, labels = next(src)
        n = int(feats['step'].shape[0])
        if n != counts[rank]:
          raise RuntimeError('data-parallel schedule expected %d windows on rank %d, the input pipeline delivered %d'
                             % (counts[rank], rank, n))
        yield feats, labels, n, sum(counts)
      else:
        yield None, None, 0, sum(counts)

  def _get_spec(self, mode, feats, labels, n, loss_scale=1.0):
    """One model (+ captured graphs) per (mode, local batch size, loss scale).  ``loss_scale`` = n_local * world /
    n_global weights this rank's batch-mean loss so that the SUM all-reduce followed by 1/world is the mean over the
    GLOBAL batch also when the ranks hold different numbers of windows (ragged final batch); 1 for equal shards."""
    key = (mode, n) if loss_scale == 1.0 else (mode, n, round(float(loss_scale), 9))
    # uint8 and float32 resident frames are read by different input kernels (a float32 episode = one whose recorded values
    # were not integral): one model per frame type, sharing the variables
    key += tuple(k for k, v in sorted(feats.items()) if isinstance(v, DeviceWindows) and not v.is_u8())
    # batches of a shuffling input (pickplace_input_fn(shuffle_windows=True)) fill their dense windows by address: feed slots of their own
    scattered = any(isinstance(v, DeviceWindows) and v.scattered for v in feats.values())
    if scattered:
      key += ('scattered',)
    # ... and so do batches of an augmenting input (pickplace_input_fn(augment=...)): their dense windows are filled by the
    # augmented gather, and no slot of theirs offers window addresses
    augmented = any(isinstance(v, DeviceWindows) and v.augmented for v in feats.values())
    if augmented:
      key += ('augmented',)
      # ... and slots of their own per set of scene extras the draws carry (occluders, sensor noise: other arena entries, another fill)
      scene = next((v.augment.scene for v in feats.values() if isinstance(v, DeviceWindows) and v.augmented), None)
      if scene is not None:
        key += ('scene:' + scene,)
      # ... and per-frame address tables when the draws carry frame sources (frame drops, camera lag: DESIGN 5.26)
      if any(isinstance(v, DeviceWindows) and v.frame_src is not None for v in feats.values()):
        key += ('frames',)
    if key in self._specs:
      return self._specs[key]
    shared = self.params.get('shared_frames')
    if shared and scattered:
      raise ValueError("params['shared_frames'] with a shuffling input (pickplace_input_fn(shuffle_windows=True)): a shuffled batch "
                       "of N windows holds about N * K distinct frames, so there is nothing to share; drop one of the two options")
    if shared and augmented:
      raise ValueError("params['shared_frames'] with an augmenting input (pickplace_input_fn(augment=...)): every window is "
                       "transformed by its own draw, so no two windows share a frame; drop one of the two options")
    fbuf, lbuf = feed.build_slots(self._device(), feats, labels,
                                  (lambda K, goal: shared_frames_capacity(shared, n, K, goal)) if shared else None)
    params = dict(self.params)
    params['_variable_store'] = self._store
    params.setdefault('use_hipgraph', self.config.use_hipgraph)
    params.setdefault('dp_form', getattr(self.config, 'dp_form', None))
    spec = self._model_fn(fbuf, lbuf, mode, params)
    spec.model.decoder.loss_scale = float(loss_scale)
    if self._store is None:
      self._store = spec.model.store.base      # (an eval / predict model of a run with ema_decay sits on the shadow view)
      self._store.initialize(seed=self.config.init_seed)
    self._restore_once()
    self._log_finetune(mode, spec.model)
    self._log_loss_shaping(spec.model)
    self._specs[key] = (spec,) + feed.adopted_slots(fbuf, lbuf, spec.model.inputs)
    return self._specs[key]

  def _restore_once(self):
    if self._restored:
      return
    self._restored = True
    ckpt = latest_checkpoint(self.model_dir) if self.model_dir else None
    if ckpt:
      load_checkpoint(self._store, ckpt)
      print('INFO: restored parameters from %s' % ckpt)
      if self.warm_start_from is not None:      # TensorFlow's rule: a run that resumes its own checkpoint is not warm-started again
        print('INFO: warm_start_from=%s is ignored: %s holds a checkpoint of its own' % (self.warm_start_from['ckpt'], self.model_dir))
    elif self.warm_start_from is not None:
      names = warm_start(self._store, self.warm_start_from)
      print('INFO: warm-started %d of %d variables from %s' % (len(names), len(self._store.shapes), self.warm_start_from['ckpt']))
    gdist.broadcast_variables(self._store)

  def _log_finetune(self, mode, model):
    """params['lr_multipliers']: one line of events.jsonl at the start of training -- trainable and frozen parameters, the cut point."""
    mults = getattr(model, 'lr_multipliers', None)
    if mode != ModeKeys.TRAIN or mults is None or self._finetune_logged:
      return
    self._finetune_logged = True
    import numpy as np
    count = lambda keep: int(sum(int(np.prod(model.store.shapes[n])) for n, mul in mults.items() if keep(mul)))
    line = {'trainable_parameters': count(lambda mul: mul != 0.0), 'frozen_parameters': count(lambda mul: mul == 0.0),
            'backward_cut': model.backward_cut, 'global_step': int(self._store.global_step.item()), 'wall_time': time.time()}
    print('INFO: fine-tuning: %(trainable_parameters)d trainable and %(frozen_parameters)d frozen parameters, backward: %(backward_cut)s' % line)
    if self.model_dir and gdist.rank() == 0:
      with open(os.path.join(self.model_dir, 'events.jsonl'), 'a') as f:
        f.write(json.dumps(line) + '\n')

  def _log_loss_shaping(self, model):
    """params['loss_shaping']: one line of events.jsonl, the option as the model took it, the first time a model with a loss is built."""
    shaping = getattr(model, 'loss_shaping', None)
    if shaping is None or self._loss_shaping_logged:
      return
    self._loss_shaping_logged = True
    line = {'loss_shaping': dict(shaping, grp_class_weights=list(shaping['grp_class_weights']) if shaping['grp_class_weights'] else None),
            'global_step': int(self._store.global_step.item()), 'wall_time': time.time()}
    print('INFO: loss shaping: %s' % json.dumps(line['loss_shaping'], sort_keys=True))
    if self.model_dir and gdist.rank() == 0:
      with open(os.path.join(self.model_dir, 'events.jsonl'), 'a') as f:
        f.write(json.dumps(line) + '\n')

  _feed_step = staticmethod(feed.feed_step)      # (fbuf, lbuf, feats, labels): one step's batch into the slots of _get_spec

  # -- public API --------------------------------------------------------------------------------
  def latest_checkpoint(self):
    return latest_checkpoint(self.model_dir)

  def get_variable_value(self, name):
    return self._store.var(name).detach().cpu().numpy()

  def get_variable_names(self):
    return list(self._store.shapes.keys())

  def train(self, input_fn, steps=None, max_steps=None):
    """``steps`` / ``max_steps`` count optimiser steps, as TensorFlow's count ``global_step``.  Under params['grad_accum_steps'] a batch is a
    micro-step and every A-th applies an optimiser step: hooks, checkpoints by step and the step count advance on those alone, and
    ``last_train_stats['micro_steps']`` counts the batches.  A group the input leaves incomplete stays in the accumulator (on the
    device, not in the checkpoint) and the next ``train()`` of this Estimator completes it."""
    world, rank = gdist.world_size(), gdist.rank()
    t0, nsteps, step, micro = time.time(), 0, None, 0
    last_runner = None
    source = input_fn()
    for feats, labels, n, n_global in self._local_batches(source, world, rank):
      if n == 0:
        # this rank has no window in this step (ragged end of the epoch): it still takes part in the gradient
        # exchange, with zeros, and applies the same update as the others
        if last_runner is None:
          raise RuntimeError('rank %d has no data in its first training step' % rank)
        last_runner.null_step()
        spec = None
      else:
        spec, fbuf, lbuf = self._get_spec(ModeKeys.TRAIN, feats, labels, n, loss_scale=n * world / float(n_global))
        self._feed_step(fbuf, lbuf, feats, labels)
        spec.train_op()
        last_runner = spec.train_op.__self__
      micro += 1
      if last_runner is not None and not last_runner.applied:      # params['grad_accum_steps']: a micro-step that applied no optimiser step
        continue
      nsteps += 1
      if (spec is not None and spec.training_hooks) or self.config.save_checkpoints_steps:
        step = int(self._store.global_step.item()) if (nsteps == 1 or step is None) else step + 1
        for h in (spec.training_hooks if spec is not None else None) or []:
          h.after_run(step, self.model_dir)
        if (self.config.save_checkpoints_steps and step % self.config.save_checkpoints_steps == 0 and rank == 0
            and self.model_dir):
          save_checkpoint(self._store, self.model_dir, self.config.keep_checkpoint_max, self.config.save_tf_bundle,
                          self.params['e2evmc_config'].batch_size if 'e2evmc_config' in self.params else None)
      if steps is not None and nsteps >= steps:
        break
      if max_steps is not None and step is not None and step >= max_steps:
        break
    if hasattr(source, 'close'):
      source.close()      # an epoch left early must not leave reader threads filling a queue nobody drains
    skipped = 0
    if micro and torch.cuda.is_available():
      torch.cuda.synchronize()
      for sp, _, _ in self._specs.values():      # a device-side error of any model that ran this epoch (input-stage timeout)
        sp.model.check_device_errors()
        skipped += check_skipped_steps(sp.model)      # ... or a run of skipped steps as long as params['skip_nonfinite'] allows
    if nsteps and world > 1 and not gdist.replicas_identical(self._store):
      # data parallel: summed gradients + a deterministic optimiser keep every replica bitwise equal; if they are not, the exchange
      # lost or raced something and rank 0's checkpoint would be one replica's opinion
      raise RuntimeError('geeco_amd: the replicas differ after %d data-parallel steps (rank %d): the gradient exchange is broken '
                         '(dp_form=%s); nothing was saved' % (nsteps, rank, getattr(self.config, 'dp_form', None) or 'three_graphs_reserve16'))
    # wall time of the input + step loop alone (the checkpoint written below is not part of the data path)
    self.last_train_stats = {'steps': nsteps, 'loop_seconds': time.time() - t0}
    if self.options.grad_accum is not None:
      self.last_train_stats['micro_steps'] = micro
    if self.options.skip_limit is not None:
      self.last_train_stats['skipped_steps'] = skipped
    if nsteps and rank == 0 and self.model_dir:
      path = save_checkpoint(self._store, self.model_dir, self.config.keep_checkpoint_max, self.config.save_tf_bundle,
                          self.params['e2evmc_config'].batch_size if 'e2evmc_config' in self.params else None)
      print('INFO: saved %s after %d steps (%.1f steps/s)' % (path, nsteps, nsteps / max(time.time() - t0, 1e-9)))
    return self

  def evaluate(self, input_fn, steps=None):
    """Streams the eval metrics of estimator.py:246-254; 'loss' = mean of per-batch losses [TF1.15]."""
    world, rank = gdist.world_size(), gdist.rank()
    sums, nb, loss_sum = {}, 0, None
    source = input_fn()
    for feats, labels, n, _ in self._local_batches(source, world, rank):
      if n == 0:
        continue
      spec, fbuf, lbuf = self._get_spec(ModeKeys.EVAL, feats, labels, n)
      self._feed_step(fbuf, lbuf, feats, labels)
      spec.train_op()
      loss_sum = spec.loss.clone() if loss_sum is None else loss_sum + spec.loss
      for k, (s, c) in spec.eval_metric_ops().items():
        if k in sums:
          sums[k][0] += s
          sums[k][1] += c
        else:
          sums[k] = [s.clone(), c]
      nb += 1
      if steps is not None and nb >= steps:
        break
    if hasattr(source, 'close'):
      source.close()
    # metric keys are fixed by the control mode (estimator.py:246-258): a rank whose shard of the eval split is empty still
    # takes part in the reduction, with zeros, instead of leaving the others waiting
    cfg = self.params.get('e2evmc_config')
    keys = sorted(sums) if sums else sorted(['cmd_ee', 'pos_ee', 'pos_obj'] + (
        ['cmd_grp'] if (cfg is None or cfg.control_mode == 'cartesian') else ['cmd_vel', 'cmd_grp']))
    if nb == 0 and world == 1:
      raise RuntimeError('evaluate(): input_fn produced no batches')
    dev = loss_sum.device if loss_sum is not None else self._device()
    zero = torch.zeros((), dtype=torch.float32, device=dev)
    vec = torch.stack([loss_sum if loss_sum is not None else zero, torch.tensor(float(nb), device=dev)] +
                      [x for k in keys for x in ((sums[k][0], torch.tensor(float(sums[k][1]), device=dev)) if k in sums
                                                 else (zero, zero))])
    if world > 1:
      torch.distributed.all_reduce(vec)
    vec = vec.double().cpu()
    for sp, _, _ in self._specs.values():
      sp.model.check_device_errors()
    if float(vec[1]) == 0.0:
      raise RuntimeError('evaluate(): input_fn produced no batches on any rank')
    out = {'loss': float(vec[0] / vec[1])}
    for i, k in enumerate(keys):
      out[k] = float(vec[2 + 2 * i] / vec[3 + 2 * i])
    out['global_step'] = int(self._store.global_step.item())
    return out

  def predict(self, input_fn):
    for batch in input_fn():
      feats = batch[0] if isinstance(batch, tuple) else batch
      n = int(next(iter(feats.values())).shape[0])
      spec, fbuf, _ = self._get_spec(ModeKeys.PREDICT, feats, None, n)
      self._feed_step(fbuf, None, feats, None)
      spec.train_op()
      torch.cuda.synchronize()
      yield {k: v.detach().cpu().numpy().copy() for k, v in spec.predictions.items()}

  def input_gradients(self, input_fn, heads=None, checkpoint_path=None):
    """d(loss)/d(frames) per batch of ``input_fn``, a generator beside ``predict()`` (saliency maps).  Every batch is
    (features, labels) of dense float arrays or tensors.  Yields numpy arrays: the gradients of ``_ModelBase.input_gradients`` ('rgb',
    'target_rgb', 'depth', 'target_depth' as the model has them), 'loss', and the predictions ``predict()`` yields.
    ``heads``: a subset of the model's head names, e.g. ('cmd_ee',) or ('cmd_grp',): the loss differentiated is the sum of those
    heads' losses with weight 1 (``LSTMDecoder.select_loss_heads``); None = the training loss.  ``checkpoint_path`` (a checkpoint
    prefix or a model_dir): parameters from there, in a store of their own, instead of the estimator's.
    The model of this pass is training-capable but takes no training option, runs eagerly and never calls the optimiser: parameters,
    optimiser state and the step counter are only read."""
    def run(model):
      model.forward(backward_too=True)
      model.backward()
      return _host_results(model, dict(model.input_gradients(), loss=model.loss), ('loss',))
    return self._input_pass('input_gradients', input_fn, heads, checkpoint_path, run)

  def attributions(self, input_fn, method='integrated_gradients', steps=16, baseline=None, noise_std=0.0, seed=0, heads=None,
                   checkpoint_path=None):
    """Integrated-gradients or SmoothGrad attributions per batch of ``input_fn``, a generator beside
    ``input_gradients()`` with its store handling, its ``heads`` and ``checkpoint_path`` and its refusals.  ``method``, ``steps``,
    ``baseline``, ``noise_std``, ``seed``: ``_ModelBase.attributions``.  Yields numpy arrays: the attributions per image input
    ('rgb', 'target_rgb', 'depth', 'target_depth' as the model has them), 'saliency' (and 'saliency_target' for goal models),
    'sample_sum', 'loss' (at the clean input), for integrated gradients 'loss_baseline' and 'completeness_gap' ([N], per sample; see
    there), and the predictions ``predict()`` yields.  The whole loop runs on the device; one read per batch."""
    from .attribution import check_attribution_arguments
    check_attribution_arguments(method, steps, noise_std, seed)

    def run(model):
      return _host_results(model, model.attributions(method, steps, baseline=baseline, noise_std=noise_std, seed=seed), ('loss', 'loss_baseline'))
    return self._input_pass('attributions', input_fn, heads, checkpoint_path, run)

  def perturbation_attributions(self, input_fn, method='occlusion', patch=None, stride=None, grid=7, keep_prob=0.5, steps=64, fill=None,
                                score='prediction', heads=None, seed=0, inputs=None, checkpoint_path=None):
    """Occlusion-sensitivity or RISE maps per batch of ``input_fn``, a generator beside ``attributions()`` with its
    store handling and its ``checkpoint_path``; every argument between: ``_ModelBase.perturbation_attributions``.  Gradient-free:
    the model of this pass is built with training=False, and labels are needed for ``score='loss'`` alone.  Yields numpy arrays:
    'saliency' [N][H][W] (one map per window), 'coverage', 'scores' [M][N], 'patch_scores' [Gy][Gx][N] (occlusion), the same with
    '_target' behind the name for goal models, and the predictions ``predict()`` yields.  The whole loop runs on the device; one
    read per batch."""
    from .perturbation import check_perturbation_arguments
    check_perturbation_arguments(method, patch, stride, grid, keep_prob, steps, score, seed)

    def run(model):
      return _host_results(model, model.perturbation_attributions(method, patch=patch, stride=stride, grid=grid, keep_prob=keep_prob, steps=steps,
                                                                  fill=fill, score=score, heads=heads, seed=seed, inputs=inputs))
    return self._input_pass('perturbation_attributions', input_fn, None, checkpoint_path, run, training=False)

  def _input_pass(self, who, input_fn, heads, checkpoint_path, run, training=True):
    """The batch loop of ``input_gradients``, ``attributions`` and ``perturbation_attributions``: the store, the refusals, one eager
    model per batch size (training-capable unless ``training`` is False: the gradient-free pass); ``run(model)`` -> the pass's numpy
    results on the loaded batch, to which the predictions are added."""
    cfg = self.params['e2evmc_config']
    goal = self._model_fn is goal_e2evmc_model_fn
    if not goal and self._model_fn is not e2evmc_model_fn:
      raise ValueError('%s: needs an Estimator built on e2evmc_model_fn or goal_e2evmc_model_fn' % who)
    if self.params.get('shared_frames'):
      raise ValueError("%s: params['shared_frames'] encodes frame slots, not windows; use dense windows for this pass" % who)
    dev = self._device()
    if checkpoint_path is not None:
      store = graph.build_store(cfg, goal, dev)
      prefix = _checkpoint_prefix(os.fspath(checkpoint_path))
      restore_for_inference(store, os.path.dirname(prefix), os.path.basename(prefix))
    else:
      if self._store is None:
        self._store = graph.build_store(cfg, goal, dev, ema=self.options.ema_decay is not None)
        self._store.initialize(seed=self.config.init_seed)
      self._restore_once()
      store = self._store
    if store.ema is not None:
      raise ValueError("%s: the estimator's store keeps averaged weights (params['ema_decay']); pass checkpoint_path= to "
                       "differentiate a checkpoint's parameters" % who)
    models = {}
    for batch in input_fn():
      feats, labels = batch if isinstance(batch, tuple) else (batch, None)
      for k, v in feats.items():
        if hasattr(v, 'pointers'):
          raise ValueError("%s: feature '%s' comes as device windows; this pass takes dense float32 batches" % (who, k))
      n = int(feats['rgb'].shape[0])
      if n not in models:
        ctor = graph.GoalE2EVMC if goal else graph.E2EVMC
        # built beside the training stack: it re-derives its weight copies on every forward and never becomes the store's primary
        primary = store.primary_stack
        models[n] = ctor(cfg, n, dev, training=training, store=store)
        if primary is None:
          store.primary_stack = None
          models[n].enc.lazy_refresh = False
        models[n].decoder.select_loss_heads(heads)
      model = models[n]
      as_t = lambda d: {k: torch.as_tensor(v) for k, v in (d or {}).items()}
      model.load_batch(as_t(feats), as_t(labels))
      out = run(model)
      out.update({k: v.detach().cpu().numpy().copy() for k, v in model.predictions().items()})
      yield out

  def replay(self, input_fn_or_episodes, checkpoint_path=None, max_frames=512, chunk_frames=None):
    """The controller's commands over whole recorded episodes, a generator beside ``predict()`` and ``input_gradients()`` (DESIGN
    5.27): one ``EpisodeReplay.replay`` result per episode of ``input_fn_or_episodes`` -- a callable that returns the episodes, or
    the episodes themselves, each a mapping as ``replay.dataset_episodes`` yields them ('rgb', 'jnt_state', the recorded per-frame
    arrays, 'target_rgb' for a goal model).  Errors are computed when the episode carries the recorded arrays of the model's heads.
    ``checkpoint_path`` (a checkpoint prefix or a model_dir): parameters from there instead of ``model_dir``'s latest checkpoint.
    The per-frame controllers go through ``EpisodeReplay``, geeco-f and 'sequence' x 'dyndiff' through ``DynamicImageReplay`` (5.29;
    ``replay_dynimg.open_replay`` picks); the pass reads the checkpoint into a store of its own and touches neither the estimator's
    parameters nor its step counter."""
    from .replay_dynimg import open_replay
    cfg = self.params['e2evmc_config']
    goal = self._model_fn is goal_e2evmc_model_fn
    if not goal and self._model_fn is not e2evmc_model_fn:
      raise ValueError('replay: needs an Estimator built on e2evmc_model_fn or goal_e2evmc_model_fn')
    if checkpoint_path is not None:
      prefix = _checkpoint_prefix(os.fspath(checkpoint_path))
      model_dir, name = os.path.dirname(prefix), os.path.basename(prefix)
    else:
      model_dir, name = self.model_dir, None
    rp = open_replay(model_dir, name, goal=goal, cfg=cfg, device=self._device(), max_frames=max_frames, chunk_frames=chunk_frames)
    label_keys = ('cmd',) if cfg.control_mode == 'cartesian' else ('vel_target', 'ee_target', 'grp_target')
    for ep in (input_fn_or_episodes() if callable(input_fn_or_episodes) else input_fn_or_episodes):
      yield rp.replay(ep, labels=hasattr(ep, 'keys') and all(k in ep for k in label_keys + ('ee_state', 'obj_state')))
