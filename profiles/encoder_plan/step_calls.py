"""Host-side record of what the models ask of the library per step: every launching ``ops`` function replaced by a recorder (name,
every argument; tensors as shape / strides / offset + the buffer whose storage they view), the planning functions left real.  No GPU.
Over profiles/graph_split/step_calls.py it also records ``backward_and_apply`` with the stream operations in between the launches
(stand-ins for torch.cuda's streams and events) and the data-parallel ``TrainStepRunner`` with a recorded exchange.
Run from a tree's root (the native library built): ``python profiles/encoder_plan/step_calls.py [--whole] > record.txt``."""
import hashlib, os, sys
sys.path.insert(0, os.getcwd())
import torch
from geeco_amd import dist as gdist, graph, ops, runtime
from geeco_amd.params import create_e2evmc_config

MAY_DECLINE = ('conv3x3_fwd_state_into', 'conv_top_bwd_into', 'conv3x3_wgrad_pair_into', 'lstm_step_heads_into', 'lstm_seq_heads_into')
LAUNCHING = sorted(n for n in dir(ops) if n.endswith('_into')) + ['slab_reduce_batch', 'adam_prepare', 'adam_tf', 'adam_tf_segments',
                                                                   'derive_conv_weights', 'sumsq_into', 'check_input_stage']
log, labels, answer, alive = [], {}, {}, []     # alive: every labelled tensor, so that no label outlives its storage


def label_tree(obj, path, seen, depth=0):
  """storage -> the first name (sorted attribute walk from the model) under which a tensor with that storage is reachable."""
  if isinstance(obj, torch.Tensor):
    alive.append(obj)
    labels.setdefault(obj.untyped_storage().data_ptr(), path)
  elif isinstance(obj, dict):
    for k in sorted(obj, key=str):
      label_tree(obj[k], '%s[%r]' % (path, k), seen, depth)
  elif isinstance(obj, (list, tuple)):
    for i, v in enumerate(obj):
      label_tree(v, '%s[%d]' % (path, i), seen, depth)
  elif hasattr(obj, '__dict__') and id(obj) not in seen and depth < 3 and not isinstance(obj, (type, Stream)):
    seen.add(id(obj))
    for k in sorted(vars(obj)):
      if (path, k) != ('enc', 'ws'):      # an alias of enc.ws_l[0] that only some trees have: the buffer is named ws_l[0] on all
        label_tree(vars(obj)[k], path + '.' + k if path else k, seen, depth + 1)


def name_tensor(t, name):
  alive.append(t)
  labels[t.untyped_storage().data_ptr()] = name


def desc(a):
  if isinstance(a, torch.Tensor):
    st = a.untyped_storage().data_ptr()
    if st not in labels:
      alive.append(a)
      labels[st] = 'tmp%d' % sum(v.startswith('tmp') for v in labels.values())
    strides = '' if a.is_contiguous() else '/strides%s' % (tuple(a.stride()),)       # (contiguous unless said)
    return '%s:%s%s%s@%d' % (labels[st], str(a.dtype)[6:], list(a.shape), strides, a.storage_offset())
  if isinstance(a, (list, tuple)):
    return '[' + ', '.join(desc(x) for x in a) + ']'
  if isinstance(a, dict):
    return '{' + ', '.join('%s=%s' % (k, desc(a[k])) for k in sorted(a)) + '}'
  if type(a).__name__ in ('HeadsFinish', 'SlabReduce'):
    return type(a).__name__
  return repr(a)


def recorder(name):
  def f(*a, **k):
    log.append('%s(%s)' % (name, ', '.join([desc(x) for x in a] + ['%s=%s' % (n, desc(k[n])) for n in sorted(k)])))
    if name == 'slab_reduce_batch':
      del a[0][:]                   # (the real one empties the list)
    elif isinstance(k.get('pending'), list):
      k['pending'].append('sum:' + name)      # (the real ones append their deferred slab sum)
    return answer.get(name, True)
  return f


for n in LAUNCHING:
  setattr(ops, n, recorder(n))


# -- stand-ins for the streams and events of torch.cuda: their operations go into the record, in order with the launches ---------
class Stream:
  count = 0

  def __init__(self, name=None, **kw):
    self.name = name or 'stream%d' % Stream.count
    Stream.count += name is None

  def wait_event(self, ev):
    log.append('%s.wait_event(%s)' % (self.name, ev.name))

  def wait_stream(self, other):
    log.append('%s.wait_stream(%s)' % (self.name, other.name))


class Event:
  count = 0

  def __init__(self, **kw):
    self.name = 'event%d' % Event.count
    Event.count += 1

  def record(self, stream=None):
    log.append('%s.record(%s)' % (self.name, stream.name if stream is not None else 'current'))


class on_stream:
  def __init__(self, stream):
    self.stream = stream

  def __enter__(self):
    log.append('enter %s' % self.stream.name)

  def __exit__(self, *exc):
    log.append('leave %s' % self.stream.name)


MAIN = Stream('main')
torch.cuda.Stream, torch.cuda.Event, torch.cuda.stream, torch.cuda.current_stream = Stream, Event, on_stream, lambda *a, **k: MAIN


# -- ... and for the exchange: every all-reduce and every wait on its work ---------------------------------------------------------
class Work:
  count = 0

  def __init__(self):
    self.name = 'work%d' % Work.count
    Work.count += 1

  def wait(self):
    log.append('%s.wait()' % self.name)


def allreduce_async(t):
  w = Work()
  log.append('%s = allreduce_async(%s)' % (w.name, desc(t)))
  return w


gdist.allreduce_async, gdist.backend = allreduce_async, lambda: 'nccl'


class Addresses:
  """Stands in for an input fed as window addresses (feed.WindowFeed.pointers())."""

  def __init__(self, name, N):
    self.table = torch.zeros(N, dtype=torch.int64)
    name_tensor(self.table, name + '.table')

  def pointers(self):
    return self


def build(cls, cfg_kw, N, size, **kw):
  cfg = create_e2evmc_config(dict(cfg_kw, img_height=size, img_width=size, batch_size=N))
  labels.clear()
  del alive[:]
  Stream.count = Event.count = Work.count = 0
  m = getattr(graph, cls)(cfg, N, 'cpu', **kw)
  label_tree(m, '', set())
  return m


def call(m, what, fn):
  log.append('-- %s' % what)
  fn()
  log.append('   _prepared=%s' % bool(getattr(m, '_prepared', False)))


def record_model(tag, cls, cfg_kw, size, decline, training=True, u8=False, N=2, **kw):
  answer.clear()
  answer.update({n: not decline for n in MAY_DECLINE})
  start = len(log)
  log.append('==== %s %dx%d %s' % (tag, size, size, 'declined' if decline else 'accepted'))
  m = build(cls, cfg_kw, N, size, training=training, **kw)
  if u8:
    for k in ('rgb', 'target_rgb'):
      m.inputs[k] = Addresses('inputs[%r]' % k, N)
  log.append('fused_bottom=%s relu_fields=%s relu_fields3=%s split_top=%s split_rgbd=%s u8_window_keys=%s' % (tuple(
      bool(getattr(m.enc, a, False)) for a in ('fused_bottom', 'relu_fields', 'relu_fields3', 'split_top')) + (m.split_rgbd, m.u8_window_keys)))
  if not training:
    for rep in range(2):
      call(m, 'forward(False) round %d' % rep, lambda: m.forward(False))
    call(m, 'check_device_errors', m.check_device_errors)
    return start
  early, late = runtime.gradient_buckets(m.store)
  g = m.store.grads
  staging = torch.zeros(sum(n for _, n in late))
  name_tensor(staging, 'staging')
  for rep in range(2):
    call(m, 'forward(True) round %d' % rep, lambda: m.forward(True))
    call(m, 'backward(adam_prepare=True)', lambda: m.backward(adam_prepare=True))
    call(m, 'apply_gradients', m.apply_gradients)
  for redirect in (False, True):
    if redirect:
      log.append('-- redirect_late_gradients -> %s' % m.redirect_late_gradients(staging, late))
    for rep in range(2):
      call(m, 'forward(True) round %d, three parts%s' % (rep, ', redirected' if redirect else ''), lambda: m.forward(True))
      call(m, "backward('upper')", lambda: m.backward('upper'))
      call(m, "backward('bottom', adam_prepare=True)", lambda: m.backward('bottom', adam_prepare=True))
      call(m, 'apply_gradients_of(early, last=False)', lambda: m.apply_gradients_of([(g[o:o + n], o, n) for o, n in early], last=False))
      if redirect:
        segs, pos = [], 0
        for o, n in late:
          segs.append((staging[pos:pos + n], o, n))
          pos += n
        call(m, 'apply_gradients_of(late from staging, g_out, last=True)', lambda: m.apply_gradients_of(segs, g_out=g, last=True))
      else:
        call(m, 'apply_gradients_of(late, last=True)', lambda: m.apply_gradients_of([(g[o:o + n], o, n) for o, n in late], last=True))
    if redirect:
      log.append('-- redirect_late_gradients(None) -> %s' % m.redirect_late_gradients(None, None))
  call(m, 'forward(True), apply_gradients without a prepared backward', lambda: m.forward(True))
  call(m, 'backward()', m.backward)
  call(m, 'apply_gradients', m.apply_gradients)
  for rep in range(2):
    call(m, 'forward(True) round %d, backward_and_apply' % rep, lambda: m.forward(True))
    call(m, 'backward_and_apply(early, late)', lambda: m.backward_and_apply(early, late))
  call(m, 'check_device_errors', m.check_device_errors)
  log.append('predictions: %s' % desc(m.predictions()))
  return start


# TrainStepRunner arguments of the data-parallel record; beside=True: dp_beside_bottom forced (a CPU model never qualifies by itself)
DP_RUNNERS = [
    ('overlap=True', dict(overlap=True), False),
    ('overlap=False', dict(overlap=False), False),
    ('reserved_cus=16', dict(reserved_cus=16), False),
    ('eager_adam=True', dict(eager_adam=True), False),
    ('capture_exchange=True', dict(capture_exchange=True), False),
    ('capture_exchange=True, dp_beside_bottom', dict(capture_exchange=True), True),
    ('capture_exchange=True, reserved_cus=16, dp_beside_bottom', dict(capture_exchange=True, reserved_cus=16), True),
]


def record_dp(tag, cls, cfg_kw, size, decline, N=2, **kw):
  """Eager steps of the data-parallel runner at one rank: the parts, the exchange and the waits in the order the runner issues them."""
  answer.clear()
  answer.update({n: not decline for n in MAY_DECLINE})
  start = len(log)
  log.append('==== dp %s %dx%d %s' % (tag, size, size, 'declined' if decline else 'accepted'))
  m = build(cls, cfg_kw, N, size, **kw)

  def at_rest(r):
    log.append('   _prepared=%s enc.reserved_cus=%r enc.late is None=%s dp_beside_bottom=%s' % (
        bool(getattr(m, '_prepared', False)), m.enc.reserved_cus, m.enc.late is None, r.dp_beside_bottom))
  for what, rkw, beside in DP_RUNNERS:
    r = runtime.TrainStepRunner(m, use_graph=False, dp=True, **rkw)
    name_tensor(r.staging, 'staging')
    log.append('-- TrainStepRunner(%s): split_adam=%s redirected=%s dp_beside_bottom=%s early_calls=%r' % (
        what, r.split_adam, r.redirected, r.dp_beside_bottom, r.early_calls))
    if beside:
      r.dp_beside_bottom = True
    for step in ('step', 'step', 'null_step'):
      log.append('-- %s.%s()' % (what, step))
      getattr(r, step)()
      at_rest(r)
    if not r.capture_exchange:      # the replayed forms' sequence, with the eager parts standing in for the graphs' replays
      log.append('-- %s._dp_step(_parts())' % what)
      r._dp_step(r._parts())
      at_rest(r)
  return start


def record_step_model(tag, cls, cfg_kw, size, decline, N=2, **kw):
  answer.clear()
  answer.update({n: not decline for n in MAY_DECLINE})
  start = len(log)
  log.append('==== %s %dx%d %s' % (tag, size, size, 'declined' if decline else 'accepted'))
  m = build(cls, cfg_kw, N, size, **kw)
  C = m.C
  frames, jnt = torch.zeros(N, size, size, C), torch.zeros(N, m.cfg.dim_jnt_state)
  reset, ctl = torch.zeros(N, dtype=torch.int32), torch.zeros(N + 1, dtype=torch.int32)
  for name, t in (('frames', frames), ('jnt', jnt), ('reset', reset), ('ctl', ctl)):
    name_tensor(t, 'arg.' + name)
  if cls == 'GoalE2EVMCStep':
    tgt = torch.zeros(1, size, size, C)
    name_tensor(tgt, 'arg.tgt_frames')
    call(m, 'encode_targets', lambda: m.encode_targets(tgt, torch.tensor([1])))
  for rep in range(2):
    call(m, 'step round %d' % rep, lambda: m.step(frames, jnt, reset, ctl))
  log.append('one_launch=%s predictions: %s' % (m.decoder.one_launch, desc(m.predictions())))
  return start


GOAL = dict(proc_obs='dynimg', proc_tgt='dyndiff', window_size=2)
SEQ = lambda t: dict(proc_obs='sequence', proc_tgt=t, window_size=2)
CASES = [
    ('E2EVMC', 'E2EVMC', dict(window_size=2), {}),
    ('geeco-f C=3', 'GoalE2EVMC', GOAL, {}),
    ('geeco-f C=3 u8', 'GoalE2EVMC', GOAL, dict(u8=True)),
    ('geeco-f C=4', 'GoalE2EVMC', dict(GOAL, img_channels=4), {}),
    ('geeco-f C=4 u8', 'GoalE2EVMC', dict(GOAL, img_channels=4), dict(u8=True)),
    ('seq_constant', 'GoalE2EVMC', SEQ('constant'), {}),
    ('seq_residual', 'GoalE2EVMC', SEQ('residual'), {}),
    ('seq_dyndiff', 'GoalE2EVMC', SEQ('dyndiff'), {}),
    ('seq_dyndiff C=4', 'GoalE2EVMC', dict(SEQ('dyndiff'), img_channels=4), {}),
    ('geeco-f split_top', 'GoalE2EVMC', dict(GOAL, dim_s_obs=256, dim_s_dyn=128, dim_s_diff=64), {}),
    ('geeco-f velocity l2', 'GoalE2EVMC', dict(GOAL, control_mode='velocity', l2_regularizer=1e-4), {}),
    ('E2EVMC velocity l2 C=4', 'E2EVMC', dict(window_size=2, control_mode='velocity', l2_regularizer=1e-4, img_channels=4), {}),
    ('E2EVMC shared_frames=8', 'E2EVMC', dict(window_size=2), dict(shared_frames=8)),
    ('seq_constant shared_frames=8', 'GoalE2EVMC', SEQ('constant'), dict(shared_frames=8)),
    ('seq_residual shared_frames=8', 'GoalE2EVMC', SEQ('residual'), dict(shared_frames=8)),
    ('E2EVMC eval', 'E2EVMC', dict(window_size=2), dict(training=False)),
    ('E2EVMC eval one-launch decoder', 'E2EVMC', dict(window_size=2), dict(training=False, one_launch_decoder=True)),
    ('geeco-f eval', 'GoalE2EVMC', GOAL, dict(training=False)),
    ('seq_residual eval', 'GoalE2EVMC', SEQ('residual'), dict(training=False)),
]
DP_CASES = [c for c in CASES if c[0] in ('E2EVMC', 'geeco-f C=3', 'geeco-f split_top')]
STEP_CASES = [
    ('E2EVMCStep', 'E2EVMCStep', dict(window_size=2), {}),
    ('E2EVMCStep one-launch decoder', 'E2EVMCStep', dict(window_size=2), dict(one_launch_decoder=True)),
    ('GoalE2EVMCStep constant', 'GoalE2EVMCStep', SEQ('constant'), dict(one_launch_decoder=True)),
    ('GoalE2EVMCStep residual', 'GoalE2EVMCStep', SEQ('residual'), {}),
]


def fold_repeats(block):
  """A call section ('-- what' up to the next) whose lines repeat an earlier section of the block is named instead of printed."""
  out, seen, i = [block[0]], {}, 1
  while i < len(block):
    j = i + 1
    while j < len(block) and not block[j].startswith('-- '):
      j += 1
    body = tuple(block[i + 1:j])
    if block[i].startswith('-- ') and len(body) > 2 and body in seen:
      out.append('%s: the %d lines of "%s"' % (block[i], len(body), seen[body]))
    else:
      seen.setdefault(body, block[i][3:])
      out.extend(block[i:j])
    i = j
  return out


def main():
  """Every case is recorded at every size with both answers.  The record names each block by line count and sha256 of its lines,
  which pins every argument; ``--whole`` prints the lines themselves (repeated call sections folded), to diff two trees with."""
  whole = '--whole' in sys.argv[1:]
  with torch.no_grad():
    for size in (256, 130, 129):
      for decline in (False, True):
        for rec, cases in ((record_model, CASES), (record_step_model, STEP_CASES), (record_dp, DP_CASES)):
          for tag, cls, cfg_kw, kw in cases:
            start = rec(tag, cls, cfg_kw, size, decline, **kw)
            block = log[start:]
            del log[start:]
            log.extend(fold_repeats(block) if whole else
                       [block[0], '%d lines, sha256 %s' % (len(block) - 1, hashlib.sha256('\n'.join(block[1:]).encode()).hexdigest())])
  print('\n'.join(log))


if __name__ == '__main__':
  main()
