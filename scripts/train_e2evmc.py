#!/usr/bin/env python
"""Training script for the end-to-end visuomotor controllers on MI355X.

Drop-in counterpart of the reference's ``scripts/train_e2evmc.py``: identical command line
(:22-124), the same ``model_dir`` protocol (``<ts>-runcmd.json``, ``e2evmc_config.json`` that wins
over the CLI on restart :229-232, ``model.ckpt-<step>*`` + ``checkpoint``, best-k ``snapshots/`` with
``snapshot_index.json`` :143-205) and the same loop: per epoch train -> evaluate -> export snapshot
(:288-291).  Only the imports differ: ``geeco_amd.estimator`` instead of ``tf.estimator``.

Data parallel: launch with ``python -m torch.distributed.run --nproc-per-node N scripts/train_e2evmc.py ...``;
``--batch_size`` stays the GLOBAL batch: each rank reads its own rank-strided share of the episodes in batches of
batch_size / world windows (geeco_amd.input_fn.pickplace_input_fn(shard=...)).
``--dataset_dir synthetic:<num_batches>`` trains on seeded synthetic windows (no dataset on disk).
"""
import argparse
import collections
import json
import os
import pprint
import re
import shutil
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))

from geeco_amd import dist as gdist                                      # noqa: E402
from geeco_amd import estimator as est                                   # noqa: E402
from geeco_amd.estimator import e2evmc_model_fn, goal_e2evmc_model_fn    # noqa: E402
from geeco_amd.input_fn import pickplace_input_fn                        # noqa: E402
from geeco_amd.params import create_e2evmc_config                        # noqa: E402
from geeco_amd.utils import load_model_config, save_model_config, save_run_command  # noqa: E402

# ---------- command line arguments (train_e2evmc.py:22-124) ----------

ARGPARSER = argparse.ArgumentParser(description='Train E2E VMC.')
_ARGS = [
    # directories
    ('--dataset_dir', str, '../data/gym-pick-pad2-cube2-v4', 'The path to the dataset (needs to conform with gym_provider).'),
    ('--split_name', str, 'default', 'The name of the data split to be used.'),
    ('--model_dir', str, '../tmp/models/geeco-f', 'The directory where the model will be stored.'),
    # model
    ('--observation_format', str, 'rgb', 'Observation data to be used (sets img_channels): rgb | rgbd.'),
    ('--control_mode', str, 'cartesian', 'Control mode of the robot: cartesian | velocity.'),
    ('--goal_condition', str, 'none', 'Conditioning mode of the reflex: none | target.'),
    ('--window_size', int, 4, 'The number of frames to process before making prediction.'),
    ('--dim_h_lstm', int, 128, 'Hidden state dimension of the LSTM.'),
    ('--dim_h_fc', int, 128, 'Output dimension of the LSTM (before decoding heads).'),
    ('--dim_s_obs', int, 256, 'Output dimension of the observation encoding.'),
    ('--dim_s_dyn', int, 256, 'Output dimension of the dynamics encoding.'),
    ('--dim_s_diff', int, 256, 'Output dimension of the target difference encoding.'),
    ('--proc_obs', str, 'sequence', 'The processing type of the frame buffer: sequence | dynimg'),
    ('--proc_tgt', str, 'constant', 'The processing type of the target frame: constant | residual | dyndiff'),
    ('--l2_regularizer', float, 0.0, 'The weight of the L2 weight regularizer. Zero disables weight regularization.'),
    ('--lambda_aux', float, 1.0, 'The weight of the auxiliary pose prediction losses. Zero disables them.'),
    # data
    ('--data_encoding', str, 'v4', 'Version of the data encoding. Available: v1 | v2 | v3 | v4'),
    # training
    ('--lr', float, 1e-4, 'The learning rate of the ADAM solver.'),
    ('--train_epochs', int, 10, 'The number of epochs to train.'),
    # snapshots
    ('--ckpt_steps', int, 10000, 'Number of steps between checkpoint saves.'),
    ('--num_last_ckpt', int, 2, 'Number of last snapshots to keep.'),
    ('--num_best_ckpt', int, 5, 'Number of best performing snapshots to keep.'),
    # memory / input threads
    ('--batch_size', int, 32, 'The number of data points (windows) per batch.'),
    ('--memcap', float, 0.8, 'Maximum fraction of memory to allocate per GPU.'),
    ('--num_threads', int, None, 'How many parallel threads to run for data fetching (reference default: 4; here, when the '
                                 'flag is absent: this rank\'s share of the host cores, input_fn.default_reader_threads).'),
    ('--prefetch_size', int, 4, 'How many batches to prefetch.'),
    ('--shuffle_buffer', int, 64, 'Number of shuffled examples to draw minibatch from.'),
    # logging
    ('--log_steps', int, 1000, 'Global steps between log output.'),
]
for _flag, _type, _default, _help in _ARGS:
  ARGPARSER.add_argument(_flag, type=_type, default=_default, help=_help)
ARGPARSER.add_argument('--debug', default=False, action='store_true', help='Enables debugging mode.')
ARGPARSER.add_argument('--initial_eval', default=False, action='store_true',
                       help='Runs an evaluation before the first training iteration.')
# the one flag the reference does not have (it has no data parallelism, train_e2evmc.py:221-224, 260-264)
ARGPARSER.add_argument('--dp_form', type=str, default=None,
                       help='Data parallel only: form of the step, one of three_graphs_reserve16 (default: exchange launched between three '
                            'replayed hipGraphs, 16 CUs left to RCCL) | three_graphs | three_graphs_serial | two_graphs (the optimiser launched eagerly behind two graphs; also two_graphs_reserve16, two_graphs_serial) | overlap (whole step '
                            'incl. both all-reduces as ONE hipGraph) '
                            '| overlap_reserve16 | overlap_reserve32 | serial.  bench.py --gpus N reports which is fastest on a node.')

ARGPARSER.add_argument('--shuffle_windows', default=False, action='store_true',
                       help='Sample-level shuffle of the training windows through a buffer of --shuffle_buffer windows (the '
                            "reference's dataset.shuffle, live in its v1-v3 pipelines); without it a batch holds consecutive windows "
                            'of one episode.  Not with --shared_frames: a shuffled batch has no frames to share.')
ARGPARSER.add_argument('--augment_shift', type=int, default=0,
                       help='Training-time augmentation, on the device: move every window (its K frames and its target frame alike) '
                            'by a random whole-pixel shift of up to this many pixels in y and in x; zeros move in.  0 = off.')
ARGPARSER.add_argument('--augment_gain', type=float, default=0.0,
                       help='... and scale each RGB channel of a window by a random gain in [1 - g, 1 + g] (0 <= g < 1).  0 = off.')
ARGPARSER.add_argument('--augment_bias', type=float, default=0.0,
                       help='... and add a random bias in [-b, b] to each RGB channel (values are clipped to [0, 1]).  0 = off.  '
                            'None of the three with --shared_frames: augmented windows share no frames.')
ARGPARSER.add_argument('--augment_noise', type=float, default=0.0,
                       help='... and add per-frame sensor noise sigma * N(0, 1) to every RGB value (0 <= sigma < 1), independent per '
                            'window, frame, pixel and channel; values are clipped to [0, 1].  0 = off.')
ARGPARSER.add_argument('--augment_occlude', type=int, default=0,
                       help='... and paint up to this many (0..4) random one-colour rectangles over each window, the same in its K '
                            'frames and its target frame (a static distractor).  0 = off.')
ARGPARSER.add_argument('--augment_occlude_size', type=float, default=0.25,
                       help="The largest side of such a rectangle as a fraction of the frame's, in (0, 1].  Not with --shared_frames "
                            'either.')
ARGPARSER.add_argument('--augment_frame_drop', type=float, default=0.0,
                       help='... and let the camera drop frames: each slot k >= 1 of a window shows, with this probability (0 <= p < 1), '
                            'the image of slot k - 1 again (drops chain).  RGB and depth alike; states and labels stay fresh.  0 = off.')
ARGPARSER.add_argument('--augment_frame_lag', type=int, default=0,
                       help='... and let the camera lag the joint encoders: per window a lag of 0..L frames, drawn uniformly, delays its '
                            "images (clamped at the episode's first frame).  0 = off.  Neither with --shared_frames.")
ARGPARSER.add_argument('--shared_frames', default=False, action='store_true',
                       help="Per-frame controllers (e2e_vmc; goal 'sequence' x 'constant' / 'residual'), one GPU, RGB: encode every "
                            'distinct frame of a batch once instead of once per window that holds it (same loss and gradients).  Needs '
                            '--batch_size <= the windows of an episode.')
ARGPARSER.add_argument('--ema_decay', type=float, default=0.0,
                       help='Keep an exponential moving average of the weights (tf.train.ExponentialMovingAverage with '
                            'num_updates = global_step: d_t = min(decay, (1 + t) / (10 + t))), updated inside the optimiser pass; '
                            'evaluation, snapshots and predictors with use_ema=True run the averaged weights.  A value in (0, 1), '
                            'e.g. 0.999; 0 = off.  Not part of the model config (e2evmc_config.json stays as the reference writes it).')
ARGPARSER.add_argument('--clip_norm', type=float, default=0.0,
                       help='Clip the gradient (L2 term included, as TF clips the gradient of the total loss) by its global norm before '
                            'the optimiser step (tf.clip_by_global_norm), on the device; events.jsonl then carries grad_norm, the norm '
                            'before clipping.  A finite number > 0, e.g. 5.0; 0 = off.  Not part of the model config.')
ARGPARSER.add_argument('--grad_accum_steps', type=int, default=1,
                       help='Apply one optimiser step per this many batches: their gradients are summed on the device and the step uses '
                            'their mean (an effective batch of A x batch_size at the memory of one batch).  Steps, --log_steps and '
                            'checkpoints count optimiser steps; a group the input leaves incomplete is completed by the next epoch, '
                            'and dropped by a restart (the accumulator is not checkpointed).  An integer >= 2; 1 = off.  One GPU.  Not '
                            'part of the model config.')
ARGPARSER.add_argument('--skip_nonfinite', default=False, action='store_true',
                       help='Skip an optimiser step whose gradient is not finite (a NaN or an infinity anywhere in it, or a norm that '
                            'overflows float32) instead of writing NaN into every weight: weights, Adam moments and averaged weights '
                            'stay as they are, the step counter still advances.  Decided on the device from the global norm; '
                            'events.jsonl then carries grad_norm and skipped_steps.  Not part of the model config.')
ARGPARSER.add_argument('--max_skipped_steps', type=int, default=None,
                       help='With --skip_nonfinite: stop training (RuntimeError, nothing saved) once this many consecutive steps were '
                            'skipped; an integer >= 1.  Default: 100.')
ARGPARSER.add_argument('--variable_stats', default=False, action='store_true',
                       help='On every logging step (--log_steps) report, per variable, the norm / largest magnitude / mean / share of exact '
                            'zeros / non-finite count of the gradient, the norm of the weights and the update-to-weight ratio: one '
                            'statistics pass on the device outside the captured step; events.jsonl carries them under "variables", the '
                            'event file as grad_norm/<var>, weight_norm/<var>, update_ratio/<var>, grad_zero_fraction/<var>.  With '
                            '--skip_nonfinite the variables that held the NaN are named.  One GPU.  Not part of the model config.')
ARGPARSER.add_argument('--variable_stats_histograms', default=False, action='store_true',
                       help='--variable_stats, and the event file also gets a magnitude histogram (by binary exponent, per sign) of every '
                            "variable's gradient and weights: gradients/<var>, weights/<var>.")
ARGPARSER.add_argument('--lr_schedule', type=str, default=None, choices=['constant', 'exponential', 'cosine', 'piecewise'],
                       help='Learning-rate schedule, evaluated on the device from its step counter (a resumed run continues it); '
                            'events.jsonl then carries learning_rate.  After --lr_warmup_steps, with u the steps since: exponential = '
                            'lr * rate^(u / decay_steps) (tf.train.exponential_decay), cosine = tf.train.cosine_decay down to alpha * lr '
                            'at decay_steps, piecewise = --lr_values between --lr_boundaries (tf.train.piecewise_constant; --lr is '
                            'ignored), constant = --lr (useful with a warm-up).  Default: the constant --lr.  Not part of the model config.')
ARGPARSER.add_argument('--lr_warmup_steps', type=int, default=0,
                       help='Linear warm-up in front of the schedule: step s < W runs lr0 * (s + 1) / W, lr0 the schedule\'s first value.')
ARGPARSER.add_argument('--lr_decay_steps', type=int, default=None, help='decay_steps of the exponential and cosine schedules (>= 1).')
ARGPARSER.add_argument('--lr_decay_rate', type=float, default=None, help='decay_rate of the exponential schedule (> 0).')
ARGPARSER.add_argument('--lr_staircase', default=False, action='store_true',
                       help='Exponential schedule: decay in steps, the exponent is floor(u / decay_steps).')
ARGPARSER.add_argument('--lr_alpha', type=float, default=0.0, help='Cosine schedule: the rate ends at alpha * lr; in [0, 1].')
ARGPARSER.add_argument('--lr_boundaries', type=str, default='',
                       help='Piecewise schedule: at most 8 strictly increasing step counts (after the warm-up), comma-separated: a,b,..')
ARGPARSER.add_argument('--lr_values', type=str, default='',
                       help='Piecewise schedule: one rate more than boundaries, comma-separated: x,y,..; value i runs while u <= boundary i.')
ARGPARSER.add_argument('--warm_start_from', type=str, default=None,
                       help='Fine-tuning: start from the weights of this checkpoint (a model_dir or a checkpoint prefix; a native .pt '
                            'file or a TF-1.15 bundle such as the published geeco_models_icra21 weights), as '
                            'tf.estimator.WarmStartSettings does: parameters only, Adam moments and the step counter start at zero.  '
                            'Ignored once --model_dir holds a checkpoint of its own.  Not part of the model config.')
ARGPARSER.add_argument('--warm_start_vars', type=str, default='.*',
                       help='With --warm_start_from: regular expression (re.search) of the variables to warm-start; the others keep '
                            'their fresh initialisation.')
ARGPARSER.add_argument('--warm_start_map', type=str, default='',
                       help='With --warm_start_from: NEW=OLD[,NEW=OLD...], prefixes of this model\'s variable names and what stands in '
                            'their place in the checkpoint, e.g. GoalVMC/ConvEncoder=VMC/ConvEncoder.')
ARGPARSER.add_argument('--lr_multipliers', type=str, default='',
                       help="Fine-tuning: 'REGEX=MULT[,REGEX=MULT...]', a learning-rate multiplier per variable (re.search on its "
                            'name, the first match wins, unmatched variables run at 1); 0 freezes a variable, and the backward stops at '
                            'the lowest layer with anything to train.  One GPU, not with --shared_frames.  Not part of the model config.')
ARGPARSER.add_argument('--freeze_encoder_bottom', default=False, action='store_true',
                       help="Shorthand for the --lr_multipliers entry '/conv[12]/=0': conv1 and conv2 of every encoder are frozen.")
ARGPARSER.add_argument('--freeze_encoders', default=False, action='store_true',
                       help="Shorthand for the --lr_multipliers entry 'Encoder/=0': only the decoder is trained.")
ARGPARSER.add_argument('--loss_grp_class_weights', type=str, default='',
                       help='Cartesian mode: a weight per gripper class for the cross-entropy of the gripper command, comma-separated in '
                            "label order (close, hold, open), e.g. 1,0.2,1 (tf.losses' weights=tf.gather(w, labels)); the mean runs over "
                            'the samples whose weight is not zero.  One GPU.  Not part of the model config.')
ARGPARSER.add_argument('--loss_label_smoothing', type=float, default=0.0,
                       help='Cartesian mode: label_smoothing of the gripper cross-entropy (tf.losses.softmax_cross_entropy), in [0, 1); '
                            '0 = off.')
ARGPARSER.add_argument('--loss_huber_delta', type=float, default=0.0,
                       help='tf.losses.huber_loss with this delta (> 0) in place of mean_squared_error on every regression head; 0 = off.')

_OBSERVATION_FORMAT_TO_CHANNELS = {'rgb': 3, 'rgbd': 4}                      # train_e2evmc.py:129-132
_GOAL_CONDITION_TO_MODEL = {'none': (e2evmc_model_fn, 'VMC'),               # train_e2evmc.py:134-137
                            'target': (goal_e2evmc_model_fn, 'GoalVMC')}


def _latest_by_ctime(model_dir, suffix):
  files = [os.path.join(model_dir, fn) for fn in os.listdir(model_dir) if fn.endswith(suffix)]
  return max(files, key=lambda fn: os.stat(fn).st_ctime)


def _export_snapshot(model_dir, eval_results, num_best_ckpt):
  """Keeps the ``num_best_ckpt`` best checkpoints by eval loss under <model_dir>/snapshots/
  (train_e2evmc.py:143-205)."""
  snapshots_dir = os.path.join(model_dir, 'snapshots')
  os.makedirs(snapshots_dir, exist_ok=True)
  index_file = os.path.join(snapshots_dir, 'snapshot_index.json')
  index = {}
  if os.path.exists(index_file):
    with open(index_file, 'r') as fp:
      index = json.load(fp)
  print('>>> Current snapshot index contains %d entries.' % len(index))
  ckpt_name = os.path.basename(est.latest_checkpoint(model_dir))
  step = int(re.search(r'\d+', ckpt_name).group(0))
  loss = float(eval_results['loss'])
  ckpt_dir = os.path.join(snapshots_dir, ckpt_name)
  os.makedirs(ckpt_dir, exist_ok=True)
  for cfg in (_latest_by_ctime(model_dir, 'runcmd.json'), _latest_by_ctime(model_dir, 'config.json')):
    shutil.copy(src=cfg, dst=ckpt_dir)
  for fn in os.listdir(model_dir):
    if fn.startswith(ckpt_name) and os.path.isfile(os.path.join(model_dir, fn)):
      shutil.copy(src=os.path.join(model_dir, fn), dst=ckpt_dir)
  with open(os.path.join(ckpt_dir, 'checkpoint'), 'w') as fp:
    fp.write('model_checkpoint_path: "%s"\n' % ckpt_name)
  print('>>> Exported current checkpoint (step=%d; loss=%.06f) to %s.' % (step, loss, ckpt_dir))
  index[ckpt_name] = {'step': step, 'loss': loss, 'dir': ckpt_dir}
  if len(index) > num_best_ckpt:
    worst = max(index.items(), key=lambda kv: kv[1]['loss'])[0]
    shutil.rmtree(index[worst]['dir'])
    info = index.pop(worst)
    print('>>> Removed worst snapshot (step=%d; loss=%.06f): %s' % (info['step'], info['loss'], info['dir']))
  with open(index_file, 'w') as fp:
    json.dump(index, fp, indent=2, sort_keys=True)
  print('>>> Saved snapshot index: %s' % index_file)
  return ckpt_dir


def estimator_params(args, e2evmc_config):
  """The Estimator's ``params`` of a command line: the model config, and the opt-ins that are not part of it."""
  params = {'e2evmc_config': e2evmc_config, 'log_steps': args.log_steps, 'debug': args.debug}
  if args.shared_frames:
    params['shared_frames'] = True
  if args.ema_decay:
    params['ema_decay'] = args.ema_decay
  if args.clip_norm:
    params['clip_norm'] = args.clip_norm
  if args.grad_accum_steps != 1:
    params['grad_accum_steps'] = args.grad_accum_steps
  if args.lr_schedule:
    params['lr_schedule'] = lr_schedule_of(args)
  if args.skip_nonfinite:
    params['skip_nonfinite'] = True if args.max_skipped_steps is None else args.max_skipped_steps
  elif args.max_skipped_steps is not None:
    raise ValueError('--max_skipped_steps %d without --skip_nonfinite: no step is ever skipped' % args.max_skipped_steps)
  if args.variable_stats_histograms:
    params['variable_stats'] = 'histograms'
  elif args.variable_stats:
    params['variable_stats'] = True
  shaping = {}
  if args.loss_grp_class_weights:
    try:
      shaping['grp_class_weights'] = [float(v) for v in args.loss_grp_class_weights.split(',')]
    except ValueError:
      raise ValueError('--loss_grp_class_weights %r: comma-separated numbers, e.g. 1,0.2,1' % args.loss_grp_class_weights)
  if args.loss_label_smoothing:
    shaping['label_smoothing'] = args.loss_label_smoothing
  if args.loss_huber_delta:
    shaping['huber_delta'] = args.loss_huber_delta
  if shaping:
    params['loss_shaping'] = shaping
  multipliers = lr_multipliers_of(args)
  if multipliers:
    params['lr_multipliers'] = multipliers
  if args.warm_start_from:
    params['warm_start_from'] = {'ckpt': args.warm_start_from, 'vars': args.warm_start_vars, 'name_map': _pairs('--warm_start_map', args.warm_start_map)}
  elif args.warm_start_map or args.warm_start_vars != '.*':
    raise ValueError('--warm_start_vars / --warm_start_map without --warm_start_from: there is no checkpoint to read')
  return params


def _pairs(flag, text):
  """'A=B,C=D' -> OrderedDict([(A, B), (C, D)]) (split at the LAST '=' of an entry: a regular expression may hold one)."""
  out = collections.OrderedDict()
  for entry in (e.strip() for e in text.split(',')):
    if not entry:
      continue
    left, eq, right = entry.rpartition('=')
    if not eq or not left or not right:
      raise ValueError('%s: %r is not of the form LEFT=RIGHT' % (flag, entry))
    out[left] = right
  return out


def lr_multipliers_of(args):
  """params['lr_multipliers'] from --lr_multipliers and its two shorthands (the shorthands first: the first match wins)."""
  out = collections.OrderedDict()
  if args.freeze_encoders:
    out['Encoder/'] = 0.0
  if args.freeze_encoder_bottom:
    out['/conv[12]/'] = 0.0
  for pattern, mul in _pairs('--lr_multipliers', args.lr_multipliers).items():
    try:
      out.setdefault(pattern, float(mul))
    except ValueError:
      raise ValueError('--lr_multipliers: %r: the multiplier %r is not a number' % (pattern, mul))
  return out


def lr_schedule_of(args):
  """params['lr_schedule'] from the --lr_* flags: the fields the chosen kind uses (the Estimator checks their values)."""
  schedule = {'kind': args.lr_schedule, 'warmup_steps': args.lr_warmup_steps}
  if args.lr_schedule in ('exponential', 'cosine'):
    schedule['decay_steps'] = args.lr_decay_steps
  if args.lr_schedule == 'exponential':
    schedule.update(decay_rate=args.lr_decay_rate, staircase=args.lr_staircase)
  if args.lr_schedule == 'cosine':
    schedule['alpha'] = args.lr_alpha
  if args.lr_schedule == 'piecewise':
    schedule['boundaries'] = [int(x) for x in args.lr_boundaries.split(',') if x.strip()]
    schedule['values'] = [float(x) for x in args.lr_values.split(',') if x.strip()]
  return schedule


def main(args):
  if args.shuffle_windows and args.shared_frames:
    # (before anything is written or initialised)
    raise SystemExit('--shuffle_windows and --shared_frames exclude each other: a shuffled batch of N windows holds about N x K '
                     'distinct frames, so there is nothing for --shared_frames to share')
  if (args.augment_shift or args.augment_gain or args.augment_bias or args.augment_noise or args.augment_occlude or
      args.augment_frame_drop or args.augment_frame_lag) and args.shared_frames:
    raise SystemExit('--augment_shift / _gain / _bias / _noise / _occlude / _frame_drop / _frame_lag and --shared_frames exclude each '
                     'other: every augmented window is transformed by its own draw, so no two windows share a frame')
  gdist.init_from_env()
  rank, world = gdist.rank(), gdist.world_size()
  os.makedirs(name=args.model_dir, exist_ok=True)
  if rank == 0:
    save_run_command(argparser=ARGPARSER, run_dir=args.model_dir)
  gpu_options = est.GPUOptions(allow_growth=True, per_process_gpu_memory_fraction=args.memcap)
  run_config = est.RunConfig(session_config=est.ConfigProto(gpu_options=gpu_options),
                             save_checkpoints_steps=args.ckpt_steps, keep_checkpoint_max=args.num_last_ckpt,
                             # checkpoints are also written as TF-1.15 tensor bundles (model.ckpt-<step>.index / .data-*),
                             # the files the reference's predictor and snapshot tooling read
                             save_tf_bundle=True, dp_form=args.dp_form)
  config_name = 'e2evmc_config'
  config_path = os.path.join(args.model_dir, '%s.json' % config_name)
  if os.path.exists(config_path):    # a previous run's config wins over the CLI (train_e2evmc.py:229-232)
    e2evmc_config = create_e2evmc_config(load_model_config(args.model_dir, config_name))
    print('>>> Loaded existing model config from %s' % (config_path,))
  else:
    e2evmc_config = create_e2evmc_config({
        'img_channels': _OBSERVATION_FORMAT_TO_CHANNELS[args.observation_format],
        'control_mode': args.control_mode, 'window_size': args.window_size, 'dim_h_lstm': args.dim_h_lstm,
        'dim_h_fc': args.dim_h_fc, 'dim_s_obs': args.dim_s_obs, 'dim_s_dyn': args.dim_s_dyn,
        'dim_s_diff': args.dim_s_diff, 'proc_obs': args.proc_obs, 'proc_tgt': args.proc_tgt,
        'l2_regularizer': args.l2_regularizer, 'lambda_aux': args.lambda_aux, 'batch_size': args.batch_size,
        'lr': args.lr})
    if rank == 0:
      save_model_config(e2evmc_config._asdict(), args.model_dir, config_name)
      print('>>> Saved model config to %s' % (config_path,))
  if world > 1:
    import torch.distributed as dist
    dist.barrier()
  model_fn, _scope = _GOAL_CONDITION_TO_MODEL[args.goal_condition]
  estimator = est.Estimator(model_fn=model_fn, model_dir=args.model_dir, config=run_config,
                            params=estimator_params(args, e2evmc_config))

  local_rank = int(os.environ.get('LOCAL_RANK', '0'))
  synthetic = args.dataset_dir.startswith('synthetic:')
  if world > 1 and not synthetic and args.batch_size % world:
    raise ValueError('--batch_size %d (the GLOBAL batch) must be divisible by the %d ranks' % (args.batch_size, world))

  # --num_threads as given; when the flag is absent, this rank's share of the host cores instead of the reference's fixed 4
  # (input_fn.default_reader_threads: epoch 1 of real-data training is reader-bound below ~13 cores per rank)
  reader_threads = args.num_threads

  def input_fn(estimator_mode):
    import torch
    dev = torch.device('cuda', local_rank)
    kw = {}
    if world > 1 and not synthetic:
      # every rank reads its own rank-strided subset of the episodes (one shuffle order agreed through rank 0's
      # seed) in batches of batch_size / world windows; ragged ends are handled by the Estimator (dp_schedule)
      seed = gdist.broadcast_int(int.from_bytes(os.urandom(4), 'little'), dev) if estimator_mode == 'train' else None
      kw = dict(shard=(rank, world), batch_size=args.batch_size // world, seed=seed)
    else:
      kw = dict(batch_size=args.batch_size, seed=None)
    return pickplace_input_fn(
        dataset_dir=args.dataset_dir, split_name=args.split_name, mode=estimator_mode, encoding=args.data_encoding,
        window_size=e2evmc_config.window_size, fetch_target=(args.goal_condition == 'target'),
        shuffle_buffer=args.shuffle_buffer, num_epochs=1, num_threads=reader_threads,
        prefetch_size=args.prefetch_size, shuffle_windows=args.shuffle_windows,
        augment=dict(shift=args.augment_shift, gain=args.augment_gain, bias=args.augment_bias, noise=args.augment_noise,
                     occlude=args.augment_occlude, occlude_size=args.augment_occlude_size, frame_drop=args.augment_frame_drop,
                     frame_lag=args.augment_frame_lag),
        # episodes are uploaded once (to THIS rank's GPU), stay there across epochs (input_fn.EPISODE_CACHE) and windows are
        # gathered in HBM; an RGB model never reads the depth stream
        device=dev,
        device_keys=('rgb',) if e2evmc_config.img_channels == 3 else ('rgb', 'depth'), **kw)
  train_input = lambda: input_fn(estimator_mode='train')
  eval_input = lambda: input_fn(estimator_mode='eval')

  if args.initial_eval:
    eval_results = estimator.evaluate(input_fn=eval_input)
    print('>>> initial eval: %s' % (eval_results,))
  for _epoch in range(args.train_epochs):
    estimator.train(input_fn=train_input)
    eval_results = estimator.evaluate(input_fn=eval_input)
    print('>>> eval: %s' % (eval_results,))
    if rank == 0:
      _export_snapshot(args.model_dir, eval_results, args.num_best_ckpt)


if __name__ == '__main__':
  print('>>> Training E2E VMC.')
  PARSED_ARGS, UNPARSED_ARGS = ARGPARSER.parse_known_args()
  print('>>> PARSED ARGV:')
  pprint.pprint(PARSED_ARGS)
  print('>>> UNPARSED ARGV:')
  pprint.pprint(UNPARSED_ARGS)
  main(PARSED_ARGS)
