"""Host-side record of what the training step asks of the library under each training option: the recorder of
profiles/encoder_plan/step_calls.py (every launching ``ops`` function replaced by a recorder of its name and every argument, stand-ins
for the streams and events) with the optimiser, clip, guard, accumulate and statistics launches added to its list.  No GPU.
Models: ``E2EVMC`` and ``GoalE2EVMC`` (dynimg) at N = 2, K = 2, 136 x 136 -- without options, one per option, and one with every option
at once -- each through ``train_step``, the beside-bottom step and the three-part step, ``variable_stats()`` where the model has it.
Run from a tree's root (the native library built): ``python profiles/train_options/step_calls.py [--whole] > record.txt``."""
import ctypes, hashlib, importlib.util, os, sys
sys.path.insert(0, os.getcwd())
spec = importlib.util.spec_from_file_location('step_calls_base', os.path.join(os.getcwd(), 'profiles', 'encoder_plan', 'step_calls.py'))
base = importlib.util.module_from_spec(spec)
spec.loader.exec_module(base)      # replaces the launching functions it lists, torch.cuda's streams and events, the exchange
from geeco_amd import ops, runtime

LAUNCHING = ['adam_prepare_schedule', 'adam_tf_ema', 'adam_tf_segments_ema', 'grad_sumsq_segments', 'clip_scale', 'adam_tf_segments_clip',
             'guard_decide', 'adam_tf_segments_guard', 'adam_tf_segments_scaled', 'grad_accumulate_segments', 'variable_stats']
LAUNCHING.append('loss_shaping')      # no launch: the struct of device pointers the shaped heads are handed, which takes CUDA tensors alone
for n in LAUNCHING:
  assert callable(getattr(ops, n)), n
  setattr(ops, n, base.recorder(n))
log, call = base.log, base.call
_desc = base.desc


def desc(a):
  if isinstance(a, ctypes.Structure):      # the schedule struct: by its fields, not by its address
    return '%s(%s)' % (type(a).__name__, ', '.join('%s=%s' % (f[0], desc(getattr(a, f[0]))) for f in a._fields_))
  if isinstance(a, ctypes.Array):      # (a long one, the opaque body of a launch plan, by its length)
    return repr(list(a)) if len(a) <= 16 else '%s[%d]' % (a._type_.__name__, len(a))
  return _desc(a)


base.desc = desc

SIZE, N = 136, 2      # (the smallest images the 2x2 state tiling takes are 129 x 129)
OPTIONS = [
    ('no options', {}),
    ('ema_decay', dict(ema_decay=0.99)),
    ('clip_norm', dict(clip_norm=1.0)),
    ('lr_schedule', dict(lr_schedule={'kind': 'cosine', 'decay_steps': 10, 'warmup_steps': 2})),
    ('skip_nonfinite', dict(skip_nonfinite=3)),
    ('lr_multipliers', dict(lr_multipliers={'LSTMDecoder/': 0.5})),
    ('lr_multipliers, encoders frozen', dict(lr_multipliers={'Encoder/': 0})),
    ('variable_stats', dict(variable_stats='histograms')),
    ('loss_shaping', dict(loss_shaping={'sample_weights': True, 'grp_class_weights': [1, 0.25, 2], 'label_smoothing': 0.1, 'huber_delta': 0.5})),
    ('grad_accum_steps', dict(grad_accum_steps=2)),
]
OPTIONS.append(('every option', {k: v for tag, kw in OPTIONS if ',' not in tag for k, v in kw.items()}))
MODELS = [('E2EVMC', 'E2EVMC', dict(window_size=2)), ('geeco-f', 'GoalE2EVMC', dict(proc_obs='dynimg', proc_tgt='dyndiff', window_size=2))]


def record(tag, cls, cfg_kw, training=True, **kw):
  base.answer.clear()
  base.answer.update({n: True for n in base.MAY_DECLINE}, loss_shaping='the shaping struct')
  start = len(log)
  log.append('==== %s' % tag)
  m = base.build(cls, cfg_kw, N, SIZE, training=training, **kw)
  log.append('options=%r' % (sorted(kw),))
  log.append('attributes: %s' % ', '.join('%s=%s' % (a, desc(getattr(m, a))) for a in (
      'ema_decay', 'clip_norm', 'skip_limit', 'lr_schedule', 'lr_multipliers', 'variable_stats_mode', 'loss_shaping', 'grad_accum', 'lr_runs',
      'backward_cut', 'clip_ws', 'clip_out', 'guard', '_lr_arg')))
  log.append('stats_plan=%s label_keys=%r inputs=%r accum=%s' % (m.stats_plan is not None, m.label_keys, sorted(m.inputs), desc(m.store.accum)))
  if not training:
    call(m, 'forward(False)', lambda: m.forward(False))
    return start
  early, late = runtime.gradient_buckets(m.store)
  g = m.store.grads
  for rep in range(3):
    call(m, 'train_step round %d' % rep, m.train_step)
  if m.stats_plan is not None:
    m.scal[0] = 1e-3      # (lr_t, which no recorded launch has written)
    call(m, 'variable_stats', lambda: log.append('   %d variables' % len(m.variable_stats())))
  if m.backward_cut == 'full':
    for rep in range(3):
      if m.grad_accum is not None:
        call(m, 'micro_step(buckets) round %d' % rep, lambda: m.micro_step((early, late)))
      else:
        call(m, 'forward(True) round %d, backward_and_apply' % rep, lambda: m.forward(True))
        call(m, 'backward_and_apply(early, late)', lambda: m.backward_and_apply(early, late))
  if m.grad_accum is None:
    for rep in range(2):
      call(m, 'forward(True) round %d, three parts' % rep, lambda: m.forward(True))
      call(m, "backward('upper')", lambda: m.backward('upper'))
      call(m, "backward('bottom', adam_prepare=True)", lambda: m.backward('bottom', adam_prepare=True))
      call(m, 'apply_gradients_of(early, last=False)', lambda: m.apply_gradients_of([(g[o:o + n], o, n) for o, n in early], last=False))
      call(m, 'apply_gradients_of(late, last=True)', lambda: m.apply_gradients_of([(g[o:o + n], o, n) for o, n in late], last=True))
    r = runtime.TrainStepRunner(m, use_graph=False)
    log.append('-- TrainStepRunner: dp=%s beside_bottom=%s accum=%r' % (r.dp, r.beside_bottom, r.accum))
  return start


def main():
  """The record names each block by line count and sha256 of its lines, which pins every argument; ``--whole`` prints the lines
  themselves (repeated call sections folded), to diff two trees with."""
  import torch
  whole = '--whole' in sys.argv[1:]
  with torch.no_grad():
    for mtag, cls, cfg_kw in MODELS:
      for otag, kw in OPTIONS:
        for training in (True, False):
          if not training and otag not in ('no options', 'loss_shaping', 'every option'):
            continue
          start = record('%s, %s%s' % (mtag, otag, '' if training else ', eval'), cls, cfg_kw, training=training, **kw)
          block = log[start:]
          del log[start:]
          log.extend(base.fold_repeats(block) if whole else
                     [block[0], '%d lines, sha256 %s' % (len(block) - 1, hashlib.sha256('\n'.join(block[1:]).encode()).hexdigest())])
  print('\n'.join(log))


if __name__ == '__main__':
  main()
