#!/usr/bin/env python
"""What episode replay costs beside stepping a batch-1 incremental predictor through the same episode.

One process, the forms alternating (scripts/_step_ab.py); e2e_vmc with seeded random weights, one ``--frames``-frame ``--size`` x
``--size`` uint8 episode at K = ``--window_size``:
  stepped_batch1:        ``E2EVMCPredictor(incremental=True)``: reset(), then predict(frame, jnt) per frame (float32 frames, the class's
                         host-side frame checks, one graph replay and one round trip per frame);
  stepped_core_uint8:    the engine below it, ``BatchedE2EVMCPredictor(num_envs=1, frame_dtype='uint8', incremental=True)``, fed the
                         recorded uint8 frames (no host-side frame check, a quarter of the upload);
  replay_resident:       ``EpisodeReplay.replay`` on the episode's frames resident in HBM (one read at the end);
  replay_dense:          the same on the dense host array (adds the upload of the frames).
Those are host-clock times around whole episodes, each ending in a device synchronise.  ``--stepped_only`` measures the two stepped
forms alone: it imports nothing of the replay, so the same file run in the parent's tree gives the baseline from the parent.
The two new kernels alone, device events around blocks of launches, each beside a plain device copy of the same bytes:
  replay_states at T x K windows (bytes: the states written + the feature / joint-state tables read once);
  replay_errors at T frames (its two launches).
Also reported: the largest difference between the replayed and the stepped predictions at this size.
Writes one JSON file (default profiles/episode_replay/replay.json).  Needs the GPU: there is no fallback.
"""
import json
import os
import statistics
import tempfile
import time

import _step_ab as ab


def host_blocks(forms, rounds, n, warm=1):
  """{name: [milliseconds per call of a block of ``n`` calls, per round]} by the host clock; every call ends in a synchronise."""
  import torch
  for fn in forms.values():
    for _ in range(warm):
      fn()
  blocks = {k: [] for k in forms}
  for _ in range(rounds):
    for k, fn in forms.items():
      torch.cuda.synchronize()
      t0 = time.perf_counter()
      for _ in range(n):
        fn()
      torch.cuda.synchronize()
      blocks[k].append((time.perf_counter() - t0) * 1e3 / n)
  return blocks


DYNIMG_MODELS = {'geeco_f': dict(proc_obs='dynimg', proc_tgt='dyndiff'), 'seq_dyndiff': dict(proc_obs='sequence', proc_tgt='dyndiff')}


def seeded_case(args, md, goal, **extra):
  """The config, one seeded uint8 episode (frames, the goal frame of a goal model, joint states) and, in ``md``, the model directory:
  the config and a checkpoint of seeded random weights."""
  import numpy as np
  from geeco_amd import estimator as est
  from geeco_amd.graph import model_variable_shapes
  from geeco_amd.params import create_e2evmc_config
  from geeco_amd.variables import VariableStore
  H, T = args.size, args.frames
  cfg = create_e2evmc_config(dict(window_size=args.window_size, img_height=H, img_width=H, **extra))
  r = np.random.default_rng(7)
  rgb = r.integers(0, 256, (T, H, H, 3), dtype=np.uint8)
  goal_frame = r.integers(0, 256, (H, H, 3), dtype=np.uint8) if goal else None
  jnt = r.standard_normal((T, cfg.dim_jnt_state)).astype(np.float32)
  json.dump(cfg._asdict(), open(os.path.join(md, 'e2evmc_config.json'), 'w'))
  st = VariableStore(model_variable_shapes(cfg, goal), 'cpu')
  st.initialize(seed=4)
  est.save_checkpoint(st, md, keep_max=1)
  return cfg, rgb, goal_frame, jnt


def episode_times(args, model, stepped, replay=None):
  """The host-clock forms.  ``stepped``: {form: (predictor, t -> the arguments of its predict)}; ``replay`` (None: the stepped forms
  alone): dict(rp=the replay object, resident=, dense= callables that replay the episode and return the result, against= the
  stepped form whose predictions the replayed ones are compared with, shape=, note= further keys of 'shape' and of
  'replay_vs_stepped').  Returns the results so far and the medians."""
  import numpy as np
  import torch
  T = args.frames

  def form(pred, feed):
    def run():
      pred.reset()
      return [pred.predict(*feed(t)) for t in range(T)]
    return run

  forms = {k: form(*v) for k, v in stepped.items()}
  results = {
      'shape': dict(size=args.size, window_size=args.window_size, frames=T, model=model, frames_dtype='uint8'),
      'timing': dict(episodes_per_block=args.steps, rounds=args.rounds,
                     method='whole episodes by the host clock, each call ending in a device synchronise, the forms alternating in one '
                            'process, medians of the blocks; kernels alone between device events, 50 launches per block'),
      'device': torch.cuda.get_device_name(torch.cuda.current_device()),
  }
  if replay is not None:
    rp = replay['rp']
    forms['replay_resident'], forms['replay_dense'] = replay['resident'], replay['dense']
    results['shape'].update(chunk_frames=rp.chunk_frames, chunk_windows=rp.chunk_windows, **replay['shape'])
    # the same commands?
    out = replay['resident']()
    pred, feed = stepped[replay['against']]
    pred.reset()
    worst, bitwise = 0.0, True
    for t in range(T):
      pred.predict(*feed(t))
      for k, v in pred._model.predictions().items():
        s = v[0].cpu().numpy()
        worst, bitwise = max(worst, float(np.abs(out[k][t] - s).max())), bitwise and np.array_equal(out[k][t], s)
    results['replay_vs_stepped'] = dict(max_abs_diff=worst, bitwise=bitwise, **replay['note'])
  blocks = host_blocks(forms, args.rounds, args.steps)
  med = {k: statistics.median(v) for k, v in blocks.items()}
  results['episode_ms'] = {k: round(v, 4) for k, v in med.items()}
  results['episode_ms_blocks'] = ab.rounded(blocks, 4)
  results['per_frame_ms'] = {k: round(v / T, 5) for k, v in med.items()}
  if replay is not None:
    results['stepped_over_replay'] = {s: round(med[s] / med['replay_resident'], 2) for s in stepped}
  return results, med


def beside_copy(args, dev, name, fn, copy_floats, copy_name='copy_same_bytes'):
  """Microseconds per call of ``fn`` and of a device copy of ``copy_floats`` floats (it reads and writes that many), alternating, 50
  launches per block: the blocks and their medians."""
  import torch
  src, dst = torch.empty(max(copy_floats, 1), device=dev), torch.empty(max(copy_floats, 1), device=dev)
  blocks = ab.alternate({name: fn, copy_name: lambda: dst.copy_(src)}, args.rounds, 50, warm=10, scale=1e3)
  return blocks, ab.medians(blocks)


def dynimg_main(args):
  """``--model geeco_f`` / ``seq_dyndiff``: the same four forms for the dynamic-image controllers -- the stepped ones are
  the NON-incremental predictors (``GoalE2EVMCPredictor``, ``BatchedGoalE2EVMCPredictor(1, frame_dtype='uint8')``; these models have
  no incremental form), the replay is ``DynamicImageReplay`` -- and the two new kernels alone: geeco_replay_images (both launches) at
  the replay's chunk beside a device copy that writes the bytes it must write, geeco_replay_states_pair at T x K windows beside a copy
  of its bytes.  ``--stepped_only`` imports nothing of the replay."""
  import numpy as np
  import torch
  from geeco_amd.batched_predictor import BatchedGoalE2EVMCPredictor
  from geeco_amd.predictor import GoalE2EVMCPredictor
  H, K, T = args.size, args.window_size, args.frames
  dev = torch.device('cuda', torch.cuda.current_device())
  with tempfile.TemporaryDirectory() as md:
    cfg, rgb, goal, jnt = seeded_case(args, md, True, **DYNIMG_MODELS[args.model])
    rgb_f, goal_f = rgb.astype(np.float32) / np.float32(255), goal.astype(np.float32) / np.float32(255)
    b1 = GoalE2EVMCPredictor(md, memcap=None, device=dev)
    b1.set_goal(goal_f)
    core = BatchedGoalE2EVMCPredictor(md, 1, memcap=None, device=dev, frame_dtype='uint8')
    core.set_goal(goal[None])
    stepped = {'stepped_batch1': (b1, lambda t: (rgb_f[t], jnt[t])), 'stepped_core_uint8': (core, lambda t: (rgb[t:t + 1], jnt[t:t + 1]))}
    if args.stepped_only:
      return ab.write(episode_times(args, args.model, stepped)[0], args.out)
    from geeco_amd import ops
    from geeco_amd.replay_dynimg import DynamicImageReplay
    rp = DynamicImageReplay(md, device=dev, max_frames=T)
    resident, goal_dev = torch.from_numpy(rgb).to(dev), torch.from_numpy(goal).to(dev)
    results, med = episode_times(args, args.model, stepped, dict(
        rp=rp, resident=lambda: rp.replay((resident, jnt), goal_frame=goal_dev, labels=False),
        dense=lambda: rp.replay((rgb, jnt), goal_frame=goal, labels=False), against='stepped_core_uint8',
        shape=dict(encoder_stacks=len(rp.encs)), note=dict(frames='all, frame 0 included')))

    # the image stage alone (both launches) at one chunk, beside a copy that writes the bytes the stage must write
    HW, F, geeco_f = H * H, rp.chunk_frames, args.model == 'geeco_f'
    n = min(F, T)
    addr = torch.from_numpy(resident.data_ptr() + np.arange(T, dtype=np.int64) * HW * 3).to(dev)
    imgs = [torch.empty(n, HW, 4, device=dev) for _ in range(3)]
    ws = ops.replay_images_ws(n, HW, dev)
    w_bytes = (3 if geeco_f else 2) * n * HW * 16
    i_blocks, i_med = beside_copy(args, dev, 'replay_images',
                                  lambda: ops.replay_images_into(imgs[0], imgs[1] if geeco_f else None, imgs[2], addr, goal_dev.view(HW, 3), T, 0, n,
                                                                 K, HW, ws), w_bytes // 4, 'copy_written_bytes')
    results.update({'replay_images_us': {k: round(v, 2) for k, v in i_med.items()}, 'replay_images_us_blocks': ab.rounded(i_blocks, 2),
                    'replay_images_windows': n, 'replay_images_written_bytes': w_bytes,
                    'replay_images_share_of_pass': round(i_med['replay_images'] * -(-T // n) / 1e3 / med['replay_resident'], 3)})
    if not geeco_f:
      d, J, cells = rp.decoder, cfg.dim_jnt_state, 4
      feat, tgt = torch.randn(T, cells, rp.dims[0], device=dev), torch.randn(T, cells, rp.dims[1], device=dev)
      jd, states = torch.from_numpy(jnt).to(dev), torch.empty(K, T, d.D, device=dev)
      s_bytes = 4 * (states.numel() + feat.numel() + tgt.numel() + jd.numel())
      s_blocks, s_med = beside_copy(args, dev, 'replay_states_pair',
                                    lambda: ops.replay_states_pair_into(states, feat, tgt, jd, T, 0, T, K, cells, rp.dims[0], rp.dims[1], J), s_bytes // 8)
      results.update({'replay_states_pair_us': {k: round(v, 2) for k, v in s_med.items()}, 'replay_states_pair_us_blocks': ab.rounded(s_blocks, 2),
                      'replay_states_pair_bytes': s_bytes})
    results['not_measured'] = ['float32 frames', 'any shape but this one', 'episodes read from disk', 'replay beside other work on the device',
                               'the stepped forms in the parent tree unless run there with --stepped_only']
    ab.write(results, args.out)


def main():
  ap = ab.arguments('episode_replay', steps_help='episodes per timed block')
  default_out = os.path.join(ab.ROOT, 'profiles', 'episode_replay', 'replay.json')
  ap.set_defaults(steps=5, out=default_out)
  ap.add_argument('--frames', type=int, default=100)
  ap.add_argument('--stepped_only', action='store_true', help='the stepped forms alone (works in a tree without the replay)')
  ap.add_argument('--model', choices=('e2e_vmc',) + tuple(DYNIMG_MODELS), default='e2e_vmc',
                  help='geeco_f / seq_dyndiff: the dynamic-image controllers (DESIGN 5.29) -> profiles/episode_replay/dynimg.json')
  args = ap.parse_args()
  import torch
  if not torch.cuda.is_available():
    raise SystemExit('episode_replay_step.py measures on the GPU; none is visible')
  if args.model != 'e2e_vmc':
    if args.out == default_out:
      args.out = os.path.join(ab.ROOT, 'profiles', 'episode_replay', 'dynimg.json' if args.model == 'geeco_f' else 'dynimg_%s.json' % args.model)
    return dynimg_main(args)

  import numpy as np
  from geeco_amd.batched_predictor import BatchedE2EVMCPredictor
  from geeco_amd.predictor import E2EVMCPredictor
  K, T = args.window_size, args.frames
  dev = torch.device('cuda', torch.cuda.current_device())
  with tempfile.TemporaryDirectory() as md:
    cfg, rgb, _, jnt = seeded_case(args, md, False)
    rgb_f = rgb.astype(np.float32) / np.float32(255)
    b1 = E2EVMCPredictor(md, memcap=None, device=dev, incremental=True)
    core = BatchedE2EVMCPredictor(md, 1, memcap=None, device=dev, frame_dtype='uint8', incremental=True)
    stepped = {'stepped_batch1': (b1, lambda t: (rgb_f[t], jnt[t])), 'stepped_core_uint8': (core, lambda t: (rgb[t:t + 1], jnt[t:t + 1]))}
    if args.stepped_only:
      return ab.write(episode_times(args, 'e2e_vmc', stepped)[0], args.out)
    from geeco_amd import ops
    from geeco_amd.replay import EpisodeReplay, error_heads
    rp = EpisodeReplay(md, device=dev, max_frames=T)
    resident = torch.from_numpy(rgb).to(dev)
    results, _ = episode_times(args, 'e2e_vmc', stepped, dict(
        rp=rp, resident=lambda: rp.replay((resident, jnt), labels=False), dense=lambda: rp.replay((rgb, jnt), labels=False),
        against='stepped_batch1', shape={}, note={}))

    # the kernels alone, each beside a copy of the same bytes (a copy reads and writes: half the bytes each way)
    d, J, cells, ch = rp.decoder, cfg.dim_jnt_state, 4, rp.ch
    feat, jd = torch.randn(T, cells, ch, device=dev), torch.from_numpy(jnt).to(dev)
    states = torch.empty(K, T, d.D, device=dev)
    s_bytes = 4 * (states.numel() + feat.numel() + jd.numel())
    k_blocks, k_med = beside_copy(args, dev, 'replay_states', lambda: ops.replay_states_into(states, feat, jd, 'plain', T, 0, T, K, cells, ch, J),
                                  s_bytes // 8)
    heads = error_heads(cfg)
    P = sum(h[1] for h in heads)
    preds, labels = torch.randn(T, P, device=dev), torch.zeros(T, P, device=dev)
    of, oe = torch.empty(T, len(heads), device=dev), torch.empty(len(heads), device=dev)
    e_bytes = 4 * (2 * preds.numel() + 2 * of.numel() + oe.numel())
    e_blocks, e_med = beside_copy(args, dev, 'replay_errors', lambda: ops.replay_errors_into(of, oe, preds, labels, T, heads), e_bytes // 8)
    results.update({
        'replay_states_us': {k: round(v, 2) for k, v in k_med.items()}, 'replay_states_us_blocks': ab.rounded(k_blocks, 2),
        'replay_states_bytes': s_bytes, 'replay_states_GBps': round(s_bytes / k_med['replay_states'] / 1e3, 1),
        'replay_states_over_copy': round(k_med['replay_states'] / k_med['copy_same_bytes'], 3),
        'replay_errors_us': {k: round(v, 2) for k, v in e_med.items()}, 'replay_errors_us_blocks': ab.rounded(e_blocks, 2),
        'replay_errors_bytes': e_bytes,
        'not_measured': ['the goal models', 'float32 frames', 'any shape but this one', 'episodes read from disk (the reader and the '
                         'upload of a new episode are outside these times)', 'replay beside other work on the device'],
    })
    ab.write(results, args.out)


if __name__ == '__main__':
  main()
