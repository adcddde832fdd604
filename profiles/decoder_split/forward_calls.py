"""Host-side equivalence of LSTMDecoder.forward / backward: every ops call with its arguments, ops mocked (no GPU).  Run from a tree's root."""
import os, sys, types
sys.path.insert(0, os.getcwd())
import torch
from geeco_amd import graph, ops, _native
from geeco_amd.variables import VariableStore
from oracle import geeco_oracle as O

log = []
def desc(a):
  if isinstance(a, torch.Tensor):
    return 'T%s/%s/@%d' % (tuple(a.shape), tuple(a.stride()), a.data_ptr() - a.untyped_storage().data_ptr())
  if isinstance(a, (list, tuple)):
    return '[' + ', '.join(desc(x) for x in a) + ']'
  if type(a).__name__ == 'HeadsFinish':
    return 'HeadsFinish'
  return repr(a)
RET = {}
def mock(name):
  def f(*a, **k):
    log.append('%s(%s)' % (name, ', '.join([desc(x) for x in a] + ['%s=%s' % (n, desc(v)) for n, v in sorted(k.items())])))
    return RET.get(name, True)
  return f
for n in ('gemm_into', 'lstm_seq_heads_into', 'lstm_step_heads_into', 'lstm_input_step_fwd_into', 'lstm_gates_fwd_into', 'heads_loss_into',
          'lstm_gates_bwd_into', 'lstm_step_bwd_into', 'colsum_into'):
  setattr(ops, n, mock(n))
ops.gemm_ws_bytes = lambda *s: 1024
ops.heads_ws_bytes = lambda *s: 1024
_native.HeadsFinish = type('HeadsFinish', (), {})

def run(tag, T, training, one_launch, ret, mode='cartesian'):
  RET.clear(); RET.update(ret)
  D, N = 1052, 3
  ocfg = O.make_config(window_size=T, control_mode=mode)
  from geeco_amd.params import create_e2evmc_config
  cfg = create_e2evmc_config(ocfg._asdict())
  st = VariableStore(O.decoder_param_shapes('dec', D, ocfg), 'cpu')
  d = graph.LSTMDecoder(st, 'dec', cfg, N, T, D, training, one_launch=one_launch)
  lab = torch.zeros(N, 8)
  d.targets, d.target_strides = [lab] * len(d.heads), [8] * len(d.heads)
  d.loss_scale = 0.5
  for rep in range(2):
    log.append('== %s call %d' % (tag, rep))
    d.forward(training)
    log.append('state one_launch=%s dz_from_heads=%s pending=%s z=%s zx=%s' % (d.one_launch, d.dz_from_heads, type(d.heads_pending).__name__,
                                                                         d.z is not None, getattr(d, 'zx', None) is not None))
    if training:
      r = d.backward()
      log.append('backward -> %r pending=%s' % (r, type(d.heads_pending).__name__))

run('train T=1 fused', 1, True, False, {})
run('train T=1 unfused', 1, True, False, {'lstm_step_heads_into': False})
run('train T=3 chain', 3, True, False, {})
run('train T=2 velocity', 2, True, False, {}, 'velocity')
run('infer T=1 fused', 1, False, True, {})
run('infer T=1 unfused', 1, False, False, {'lstm_step_heads_into': False})
run('infer T=3 chain', 3, False, False, {})
run('infer T=3 one-launch', 3, False, True, {})
run('infer T=3 one-launch declined', 3, False, True, {'lstm_seq_heads_into': False})
print('\n'.join(log))
