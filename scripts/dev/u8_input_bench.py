"""Dev: the input stage alone from resident uint8 frames (geeco_goal_dynimgs_u8_fwd) against the fp32 form, N=32 K=16 256x256 by default (the
RGB big-grid kernels).  --depth: the RGB-D instantiations; --N 1: the 256-thread kernels of small batches.  Without --depth
the plain dynamic image (dynimg_wsum3_kernel + dynimg_norm_kernel) of the same windows is timed too.  --digest: the line ends
with a SHA-256 of the three outputs of the uint8 form and of the fp32 form (taken after the warm-up calls, on the seeded inputs):
two library builds compute the same bits exactly when these agree."""
import argparse, hashlib, os, sys
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', '..'))
import numpy as np, torch
from geeco_amd import ops
dev = torch.device('cuda', 0)
ap = argparse.ArgumentParser()
ap.add_argument('--N', type=int, default=32)
ap.add_argument('--depth', action='store_true')
ap.add_argument('--digest', action='store_true')
args = ap.parse_args()
N, K, H, W = args.N, 16, 256, 256
HW, fe = H * W, H * W * 3
r = np.random.default_rng(0)
torch.manual_seed(0)
eps = [torch.tensor(r.integers(0, 256, size=(100, fe), dtype=np.uint8), device=dev) for _ in range(N)]
tg = [torch.tensor(r.integers(0, 256, size=(1, fe), dtype=np.uint8), device=dev) for _ in range(N)]
win = torch.tensor([e.data_ptr() + int(r.integers(0, 84)) * fe for e in eps], dtype=torch.int64, device=dev)
tpt = torch.tensor([t.data_ptr() for t in tg], dtype=torch.int64, device=dev)
rgb = torch.rand(N, K, H, W, 3, device=dev)
tgt = torch.rand(N, H, W, 3, device=dev)

ws2 = ops.goal_dynimgs_ws(N, HW, dev)
out = [torch.empty(N, H, W, 4, device=dev) for _ in range(3)]
big = torch.empty(256 << 20, dtype=torch.uint8, device=dev)      # flushes the caches between samples
def timeit(fn, reps=30):
  ts = []
  for _ in range(reps):
    big.zero_()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(); fn(); b.record(); torch.cuda.synchronize()
    ts.append(a.elapsed_time(b) * 1e3)
  ts.sort()
  return ts[len(ts) // 2], ts[2], ts[-3]
kw = {}
if args.depth:
  kw = dict(depth=torch.rand(N, K, H, W, 1, device=dev), tgt_depth=torch.rand(N, H, W, 1, device=dev), dsample_stride=K * HW,
            dframe_stride=HW)
u8 = lambda: ops.goal_dynimgs_u8_into(out[0], out[1], out[2], win, tpt, K, N, HW, ws2, **kw)
f32 = lambda: ops.goal_dynimgs_into(out[0], out[1], out[2], rgb, tgt, K, N, HW, ws2, K * fe, fe, **kw)
ws = ops.dynimg_ws(N, HW * 4, dev)
plain = lambda: ops.dynimg_into(out[1], rgb, K, N, HW, 3, 4, ws, K * fe, fe)
for _ in range(3):
  u8(); f32(); plain()
def digest(fn):
  fn()
  h = hashlib.sha256()
  for o in out:
    h.update(o.cpu().numpy().tobytes())
  return h.hexdigest()
sha = ' | sha256 uint8 %s fp32 %s' % (digest(u8), digest(f32)) if args.digest else ''
print('%s N=%d%s: uint8 by address %.1f us (p10 %.1f p90 %.1f) | fp32 windows %.1f us (one launch each)%s%s' %
      ((os.environ.get('GEECO_LIB', 'default'), N, ' rgbd' if args.depth else '') + timeit(u8) + timeit(f32)[:1] +
       ('' if args.depth else ' | plain dynimg %.1f us (two launches)' % timeit(plain)[0], sha)))
