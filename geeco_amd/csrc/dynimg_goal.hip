// The goal model's one-pass input stage: the buffer image, the pair image and the current frame's padded copy in one launch
// (the plain dynamic image: dynimg.hip).  From frame_ingest.h: u8x4_unit, the Newton form of the uint8 conversion.
#include "dynimg_internal.h"
#include "frame_ingest.h"
#include <vector>

// 4 pixels = 12 bytes = three dwords of a uint8 RGB frame -> the three float4 the fp32 path loads
__device__ __forceinline__ void load_u8_unit(const unsigned char* frame, long long u, f32x4& v0, f32x4& v1, f32x4& v2) {
  // (the frame address comes out of a table in memory: say that it is global memory, or the compiler emits flat loads)
  typedef const __attribute__((address_space(1))) unsigned int* gptr;
  gptr s = (gptr)(reinterpret_cast<const unsigned int*>(frame) + u * 3);
  // non-temporal: the window is read once; what should stay in L2 / the memory-side cache are the three images this kernel writes
  // for conv1 (measured, same box: uint8 input stage 73 -> 58 us, fp32 131-136 -> 111-116 us in the step)
  const unsigned int b0 = __builtin_nontemporal_load(s), b1 = __builtin_nontemporal_load(s + 1), b2 = __builtin_nontemporal_load(s + 2);
  v0 = u8x4_unit(b0);
  v1 = u8x4_unit(b1);
  v2 = u8x4_unit(b2);
}

// ------------------------------------------------------------------------------------------------------------------
// The goal model's input stage in ONE pass (round 5; rounds 3-4: the K-frame pass + a normalisation launch that re-read and
// re-wrote both images: 134 MB of the stage's 662 MB).  A thread keeps its pixels of BOTH images in registers across the
// per-sample min / max, then normalises and stores them once:
//   * thread = UPT units of 4 pixels (units u, u + THREADS, ...: consecutive lanes read consecutive 48 B), block = THREADS
//     threads; a sample is covered by bps = ceil(HW / 4 / (THREADS * UPT)) blocks with consecutive block indices;
//   * block min / max of the two images -> ONE lane publishes them as write-through (sc1) stores into the block's slot of the
//     sample's partial array, waits for those stores, and counts the block in with an agent-scope atomic add (memory side); the
//     same wave polls the sample's counter (sc1 loads) until its bps blocks are in, then fetches the bps slots with sc1 loads
//     and reduces them -- every hand-off byte is written through and read past this XCD's L2 (per-XCD L2s are not coherent), so
//     no L2 write-back / invalidate is needed; critical path = one store, one atomic, one load latency;
//   * a block waits only for the OTHER BLOCKS OF ITS SAMPLE (not a grid barrier): they run the same K-frame pass and arrive
//     together; blocks of a sample have consecutive indices and workgroups start in index order, so every sample ahead of a
//     partially started one is complete or fully resident: the wait cannot deadlock however many blocks fit on the chip.
//     In-order start of workgroups is how the dispatcher of every CDNA part behaves, NOT a documented guarantee (CU masking, a
//     partitioned device or a co-resident persistent kernel could starve a sample's last blocks).  So the wait is BOUNDED
//     (g_wait_polls polls, seconds) and an expired wait is LOUD: the block counts itself into the sample's sticky `timeouts`
//     word and normalises with NaN, and geeco_goal_dynimgs_timeouts() (which the host calls wherever it synchronises anyway)
//     reports the count.  The word is what makes it loud: the NaN images are visible as such (endpoints), but conv1's ReLU
//     -- max(x, 0) returns 0 for a NaN -- would let a finite loss come out of them.  Nothing ever continues on stale min / max.  A workspace that has seen a timeout stays poisoned (its counters are no longer zero
//     between calls) until the caller zero-fills it again;
//   * ordering of the hand-off, at the hardware level (the C++ model has no word for "write-through store"): the slot stores
//     and the counter add are agent-scope atomics = sc1 accesses that complete at the memory side, past the non-coherent
//     per-XCD L2s; the producer drains its slot stores (s_waitcnt vmcnt(0)) BEFORE it issues the add; on the consumer side
//     every lane of the polling wave takes the final count from lane 0 through readfirstlane and the ADDRESS of its slot loads
//     is computed from that count (+ count >> 31, i.e. + 0), so the slot loads are issued behind the poll that saw the full
//     count by data dependence -- for all 64 lanes, for the compiler and for the wave -- not by reconvergence and without a
//     fence (a workgroup-scope acquire fence here measured +2...3 us in the step: it drains the wave's prefetched frame loads
//     of the NEXT sample, which the hand-off does not depend on).  Agent-scope release / acquire (buffer_wbl2 / buffer_inv
//     sc1 per block) would write back and invalidate an XCD's whole L2 for four floats that never live in it;
//   * the LAST block of a sample to leave zeroes the sample's two counters again: every call finds and leaves them zero (the
//     slots need no reset: every block rewrites its own before it counts itself in).
// The arithmetic per pixel is that of dynimg_wsum3_kernel + dynimg_norm_kernel (dynimg.hip; same sums in the same order, (D - min) / range
// with the IEEE division): bitwise the same images.
// ------------------------------------------------------------------------------------------------------------------
struct DynCtl {           // per sample: the two counters, on a 64-byte line of their own; zero between calls.  Behind the N
  unsigned arrive, depart;      // control blocks: N x bps slots of {min, max of the buffer image, min, max of the pair image}
  unsigned timeouts;            // sticky: blocks of this sample whose wait expired (never reset by the kernels)
  unsigned pad[13];
};

// polls of the sample counter before a block gives up (s_sleep 4 + one sc1 load each: 2^22 polls are seconds; the blocks of a
// sample arrive within microseconds of each other).  geeco_goal_dynimgs_set_wait_polls: tests set 0, so that every block that is
// not the last of its sample to arrive reports a timeout.
static unsigned g_wait_polls = 1u << 22;

// the wait itself: lane 0 polls, every lane of the wave gets the final count
__device__ __forceinline__ unsigned dyn_wait_for_sample(DynCtl* c, unsigned got, unsigned bps, unsigned polls, bool lane0) {
  if (lane0) {
    for (unsigned spin = 0; got < bps && spin < polls; ++spin) {
      __builtin_amdgcn_s_sleep(4);
      got = __hip_atomic_load(&c->arrive, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    if (got < bps) __hip_atomic_fetch_add(&c->timeouts, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  return __builtin_amdgcn_readfirstlane(got);
}

// a wave-uniform address as such (two SGPRs): loads from it + a 32-bit per-lane offset take the scalar-base form and need one VGPR
// of address instead of a 64-bit pair per load (which the compiler precomputes per frame of the unrolled ring and spills)
__device__ __forceinline__ const char* dyn_uniform(const void* q) {
  const unsigned long long v = (unsigned long long)q;
  const unsigned lo = __builtin_amdgcn_readfirstlane((unsigned)v), hi = __builtin_amdgcn_readfirstlane((unsigned)(v >> 32));
  return reinterpret_cast<const char*>(((unsigned long long)hi << 32) | lo);
}

// Publish and arrive, ONE lane of the block (its own wave's min / max in hand, behind the barrier that completes red[]): folds the
// waves' partials and publishes the block's four numbers as write-through stores into its slot of the sample's partial array,
// waits for those stores, then counts the block in (agent-scope atomic add, memory side).  Returns the sample's count with this
// block in it.
template <int NW>
__device__ __forceinline__ unsigned dyn_publish_arrive(DynCtl* c, f32x4* slots, int b, const float (&red)[NW][4], float mn1, float mx1,
                                                       float mn2, float mx2) {
  for (int i = 1; i < NW; ++i) {
    mn1 = fminf(mn1, red[i][0]); mx1 = fmaxf(mx1, red[i][1]);
    mn2 = fminf(mn2, red[i][2]); mx2 = fmaxf(mx2, red[i][3]);
  }
  float* sp = reinterpret_cast<float*>(slots + b);      // (formed here, behind the fold: as the kernels always had it)
  __hip_atomic_store(sp + 0, mn1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);      // (agent-scope relaxed = sc1 write-through stores)
  __hip_atomic_store(sp + 1, mx1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  __hip_atomic_store(sp + 2, mn2, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  __hip_atomic_store(sp + 3, mx2, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  return __hip_atomic_fetch_add(&c->arrive, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) + 1u;
}

// Collect, ONE wave of the block (lane = its lane index; got = the sample's count as lane 0 last saw it): polls the sample's
// counter; once all bps blocks are in, lanes 0..bps-1 fetch the slots (sc1 loads: served past this XCD's L2) and a wave
// reduction gives the sample's min / max -- one store, one atomic and one load latency on the critical path (the first form
// used four returning atomic max + four read-backs: ~15 us of latency).  Leaves s_norm = {min1, range1, min2, range2} for the
// block (the caller's barrier publishes it) and counts the block out.  The other blocks of the sample run the same pass over
// the same number of frames: they are at most a few us behind.
__device__ __forceinline__ void dyn_collect(DynCtl* c, const f32x4* slots, unsigned got, int bps, unsigned polls, int lane,
                                            float (&s_norm)[4]) {
  got = dyn_wait_for_sample(c, got, (unsigned)bps, polls, lane == 0);
  const bool expired = got < (unsigned)bps;
  slots += got >> 31;      // + 0 (a count never has bit 31 set): the slot loads below carry an ADDRESS dependency on the final count
  f32x4 q = {INFINITY, -INFINITY, INFINITY, -INFINITY};
  for (int i = lane; i < bps; i += 64) {
    const float* sp = reinterpret_cast<const float*>(slots + i);
    const float q0 = __hip_atomic_load(sp + 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const float q1 = __hip_atomic_load(sp + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const float q2 = __hip_atomic_load(sp + 2, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const float q3 = __hip_atomic_load(sp + 3, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    q.x = fminf(q.x, q0); q.y = fmaxf(q.y, q1); q.z = fminf(q.z, q2); q.w = fmaxf(q.w, q3);
  }
  const float a1 = wave_reduce_min(q.x), b1 = wave_reduce_max(q.y), a2 = wave_reduce_min(q.z), b2 = wave_reduce_max(q.w);
  if (lane == 0) {
    s_norm[0] = a1; s_norm[1] = expired ? NAN : b1 - a1 + 1e-6f;      // graph.py:49 (expired wait: NaN images, never stale ones)
    s_norm[2] = a2; s_norm[3] = expired ? NAN : b2 - a2 + 1e-6f;
    // leave: the last block out zeroes the two counters for the next call (every block has read the slots by then)
    if (__hip_atomic_fetch_add(&c->depart, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == (unsigned)bps - 1u) {
      __hip_atomic_exchange(&c->arrive, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      __hip_atomic_exchange(&c->depart, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
  }
}

// ------------------------------------------------------------------------------------------------------------------
// The per-lane work of the stage, once for both kernels below.  A lane owns UPT unit slots of 4 pixels; what differs between the
// kernels is how many slots, how many frames of loads are in flight, and what happens between the samples of a block.
// Every helper is inlined and indexes its arrays with constants only (#pragma unroll): a dynamic index would send the
// accumulators to scratch.  dyn_to_units holds barriers, so its callers (dyn_last_frame, dyn_emit) are called by EVERY thread of
// a block, on block-uniform paths, and branch on `live` only behind it.
// ------------------------------------------------------------------------------------------------------------------
// Where a lane stands for unit slot j of a block whose first unit is ub.  Two register layouts of the 12 RGB floats of a slot
// (the depths, one float4 per unit, always belong to unit ub + j * THREADS + tid):
//   unit layout (U8 source): x[c] = c-th float4 of unit ub + j * THREADS + tid (one dwordx3 of bytes per lane and frame);
//   flat layout (fp32 source): x[c] = float4 number (j * 3 + c) * THREADS + tid of the block's stretch of the frame, so
//     every load instruction of a wave reads 1 KiB contiguous (the unit layout reads 16 of every 48 bytes per instruction:
//     three times the cache-line requests; measured on the first form of this kernel).  Sums, products and min / max do not
//     care which pixel a float belongs to; the three arrays that are stored per pixel (current frame, both images) go through
//     an LDS transposition (dyn_to_units) once, after the frame loop.
// Threads past the end of a ragged last block read the frame's last unit / float4 again and drop what they computed: the frame
// loop has no branch.  Positions are 32-bit BYTE offsets from wave-uniform frame addresses: one VGPR each, and the loads take
// the scalar-base form; a frame is at most HW * 16 bytes, checked by the launcher to stay below 2^31.
struct DynLane {
  unsigned uc, fo[3];      // unit index (clamped); byte offset of the slot's c-th float4 in the frame (flat layout)
  bool live, flive[3];     // the unit / the c-th float4 lies inside the frame
};

template <int THREADS, bool U8>
__device__ __forceinline__ DynLane dyn_lane(long long ub, int j, int tid, long long U) {
  DynLane l;
  const long long u = ub + (long long)j * THREADS + tid;
  l.live = u < U;
  l.uc = (unsigned)(l.live ? u : U - 1);
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const long long f = ub * 3 + (long long)(j * 3 + c) * THREADS + tid;
    l.flive[c] = U8 ? l.live : f < 3 * U;
    l.fo[c] = (unsigned)((f < 3 * U ? f : 3 * U - 1) * 16);
  }
  return l;
}

// 16 bytes, non-temporal (global address space said explicitly: a pointer rebuilt from integers would load "flat")
__device__ __forceinline__ f32x4 dyn_ld4(const void* q) {
  typedef const __attribute__((address_space(1))) f32x4* gptr;
  return __builtin_nontemporal_load((gptr)q);
}

// flat layout -> unit layout of one slot's three float4 through LDS (fp32 source only; every thread of the block takes part)
template <int THREADS, bool U8>
__device__ __forceinline__ void dyn_to_units(int tid, f32x4& x0, f32x4& x1, f32x4& x2) {
  if constexpr (!U8) {
    __shared__ f32x4 tbuf[THREADS * 3];
    __syncthreads();
    tbuf[tid] = x0; tbuf[THREADS + tid] = x1; tbuf[2 * THREADS + tid] = x2;
    __syncthreads();
    x0 = tbuf[3 * tid]; x1 = tbuf[3 * tid + 1]; x2 = tbuf[3 * tid + 2];
  }
}

// frame t of sample n (wbase = p.win[n], U8 only) / the sample's target frame: three RGB float4 and, with DEPTH, the depths
template <bool DEPTH, bool U8>
__device__ __forceinline__ void dyn_load_frame(const DynParams& p, const unsigned char* wbase, int n, int t, const DynLane& l, f32x4 (&v)[4]) {
  if (U8) {
    load_u8_unit(wbase + (long long)t * p.HW * 3, l.uc, v[0], v[1], v[2]);
  } else {
    const char* src = dyn_uniform(p.frames + (long long)n * p.sample_stride + (long long)t * p.frame_stride);
    v[0] = dyn_ld4(src + l.fo[0]); v[1] = dyn_ld4(src + l.fo[1]); v[2] = dyn_ld4(src + l.fo[2]);
  }
  if (DEPTH) v[3] = dyn_ld4(dyn_uniform(p.depth + (long long)n * p.dsample_stride + (long long)t * p.dframe_stride) + l.uc * 16u);
}

template <bool DEPTH, bool U8>
__device__ __forceinline__ void dyn_load_target(const DynParams& p, int n, const DynLane& l, f32x4 (&g)[4]) {
  if (U8) {
    load_u8_unit(p.tgt_u8[n], l.uc, g[0], g[1], g[2]);
  } else {
    const char* ts = dyn_uniform(p.tgt + (long long)n * p.HW * 3);
    g[0] = dyn_ld4(ts + l.fo[0]); g[1] = dyn_ld4(ts + l.fo[1]); g[2] = dyn_ld4(ts + l.fo[2]);
  }
  if (DEPTH) g[3] = dyn_ld4(dyn_uniform(p.tgt_depth + (long long)n * p.HW) + l.uc * 16u);
}

template <bool DEPTH>
__device__ __forceinline__ void dyn_axpy(f32x4 (&X)[4], float w, const f32x4 (&v)[4]) {
  X[0] += w * v[0]; X[1] += w * v[1]; X[2] += w * v[2];
  if (DEPTH) X[3] += w * v[3];
}

// Frames 0 .. K-2 into the buffer image A, software-pipelined: a ring of UNR frames of staging registers; a frame's registers are
// refilled with the frame UNR ahead as soon as its products are taken, so a wave always has ~UNR * UPT * 3 loads in flight.
// mid() is called once, by every thread, about half-way through the frames (block-uniform: it may hold barriers).
template <bool DEPTH, bool U8, int UNR, int UPT, class Mid>
__device__ __forceinline__ void dyn_walk_frames(const DynParams& p, const unsigned char* wbase, int n, const DynLane (&l)[UPT],
                                                f32x4 (&A)[UPT][4], Mid&& mid) {
  const int KM = p.K - 1;
  const int groups = KM / UNR;
  const int gmid = groups >> 1;
  bool called = false;
  if (groups > 0) {
    f32x4 v[UNR][UPT][4];
#pragma unroll
    for (int k = 0; k < UNR; ++k)
#pragma unroll
      for (int j = 0; j < UPT; ++j) dyn_load_frame<DEPTH, U8>(p, wbase, n, k, l[j], v[k][j]);
    for (int g = 0; g + 1 < groups; ++g) {      // steady state: no condition inside but mid's
      if (g == gmid) {
        mid();
        called = true;
      }
#pragma unroll
      for (int k = 0; k < UNR; ++k) {
        const float w = p.alpha[g * UNR + k];
#pragma unroll
        for (int j = 0; j < UPT; ++j) dyn_axpy<DEPTH>(A[j], w, v[k][j]);
#pragma unroll
        for (int j = 0; j < UPT; ++j) dyn_load_frame<DEPTH, U8>(p, wbase, n, (g + 1) * UNR + k, l[j], v[k][j]);
        __builtin_amdgcn_sched_barrier(0);      // keep this order: (consume frame k, refill its registers), next k -- the scheduler
      }                                         // otherwise sinks all refills behind the last wait of the round
    }
#pragma unroll
    for (int k = 0; k < UNR; ++k) {
      const float w = p.alpha[(groups - 1) * UNR + k];
#pragma unroll
      for (int j = 0; j < UPT; ++j) dyn_axpy<DEPTH>(A[j], w, v[k][j]);
    }
  }
  if (!called) mid();
  for (int t = groups * UNR; t < KM; ++t) {     // K - 1 not a multiple of UNR: the remaining frames one by one
    const float w = p.alpha[t];
#pragma unroll
    for (int j = 0; j < UPT; ++j) {
      f32x4 v[4];
      dyn_load_frame<DEPTH, U8>(p, wbase, n, t, l[j], v);
      dyn_axpy<DEPTH>(A[j], w, v);
    }
  }
}

// 4 pixels of a channel-padded [N][HW][4] image: where the lane's unit lies, and its three RGB float4 interleaved with its four
// fourth-channel values
__device__ __forceinline__ f32x4* dyn_pixels(float* img, const DynParams& p, int n, const DynLane& l) {
  return reinterpret_cast<f32x4*>(img + ((long long)n * p.HW + (long long)l.uc * 4) * 4);
}

__device__ __forceinline__ void dyn_store_pixels4(f32x4* dst, const f32x4 v0, const f32x4 v1, const f32x4 v2, const f32x4 v3) {
  dst[0] = f32x4{v0.x, v0.y, v0.z, v3.x};
  dst[1] = f32x4{v0.w, v1.x, v1.y, v3.y};
  dst[2] = f32x4{v1.z, v1.w, v2.x, v3.z};
  dst[3] = f32x4{v2.y, v2.z, v2.w, v3.w};
}

// The window's last frame = the current frame: the last term of A, the ConvEncoder's input (its padded copy goes to p.last) and
// the first term of the pair image D, summed in the order of the two-frame pass: 0 + alpha2[0] * current, + alpha2[1] * target
template <bool DEPTH, bool U8, int THREADS, int UPT>
__device__ __forceinline__ void dyn_last_frame(const DynParams& p, const unsigned char* wbase, int n, int tid, const DynLane (&l)[UPT],
                                               f32x4 (&A)[UPT][4], f32x4 (&D)[UPT][4]) {
  const float w = p.alpha[p.K - 1], w0 = p.alpha2[0], w1 = p.alpha2[1];
  f32x4 c[UPT][4], g[UPT][4];
#pragma unroll
  for (int j = 0; j < UPT; ++j) {
    c[j][3] = g[j][3] = f32x4{0.f, 0.f, 0.f, 0.f};
    dyn_load_frame<DEPTH, U8>(p, wbase, n, p.K - 1, l[j], c[j]);
    dyn_load_target<DEPTH, U8>(p, n, l[j], g[j]);
  }
#pragma unroll
  for (int j = 0; j < UPT; ++j) {
    dyn_axpy<DEPTH>(A[j], w, c[j]);
    dyn_axpy<DEPTH>(D[j], w0, c[j]);
    dyn_axpy<DEPTH>(D[j], w1, g[j]);
  }
#pragma unroll
  for (int j = 0; j < UPT; ++j) {
    dyn_to_units<THREADS, U8>(tid, c[j][0], c[j][1], c[j][2]);
    if (l[j].live) dyn_store_pixels4(dyn_pixels(p.last, p, n, l[j]), c[j][0], c[j][1], c[j][2], c[j][3]);
  }
}

// one slot's part of the lane's min / max of both images
template <bool DEPTH>
__device__ __forceinline__ void dyn_lane_minmax(const DynLane& l, const f32x4 (&A)[4], const f32x4 (&D)[4], float& mn1, float& mx1,
                                                float& mn2, float& mx2) {
#pragma unroll
  for (int q = 0; q < (DEPTH ? 4 : 3); ++q) {
    if (!(q < 3 ? l.flive[q] : l.live)) continue;
    const f32x4 a = A[q], d = D[q];
    mn1 = fminf(fminf(mn1, fminf(a.x, a.y)), fminf(a.z, a.w));
    mx1 = fmaxf(fmaxf(mx1, fmaxf(a.x, a.y)), fmaxf(a.z, a.w));
    mn2 = fminf(fminf(mn2, fminf(d.x, d.y)), fminf(d.z, d.w));
    mx2 = fmaxf(fmaxf(mx2, fmaxf(d.x, d.y)), fmaxf(d.z, d.w));
  }
}

// One image of one slot: normalise in place, transpose, store.  (One image at a time: half the live registers of both together.)
template <bool DEPTH, bool U8, int THREADS>
__device__ __forceinline__ void dyn_emit(f32x4 (&X)[4], float m, float r, float* img, const DynParams& p, int n, int tid, const DynLane& l) {
#pragma unroll
  for (int q = 0; q < (DEPTH ? 4 : 3); ++q) {
    X[q].x = (X[q].x - m) / r; X[q].y = (X[q].y - m) / r; X[q].z = (X[q].z - m) / r; X[q].w = (X[q].w - m) / r;
  }
  dyn_to_units<THREADS, U8>(tid, X[0], X[1], X[2]);
  if (!l.live) return;
  dyn_store_pixels4(dyn_pixels(img, p, n, l), X[0], X[1], X[2], DEPTH ? X[3] : f32x4{0.f, 0.f, 0.f, 0.f});
}

// One sample per block, UPT unit slots per thread.
template <bool DEPTH, bool U8, int THREADS, int UPT>
__global__ __launch_bounds__(THREADS) void dynimg_goal_onepass_kernel(const DynParams p, DynCtl* ctl, int bps, unsigned polls) {
  constexpr int NW = THREADS / 64;
  const int n = blockIdx.x / bps, b = blockIdx.x - n * bps;
  const int tid = threadIdx.x;
  [[maybe_unused]] const unsigned char* wbase = U8 ? p.win[n] : nullptr;
  const long long U = p.HW >> 2;             // units of 4 pixels per frame
  const long long ub = (long long)b * (THREADS * UPT);      // first unit of this block
  f32x4 A[UPT][4], D[UPT][4];      // buffer image / pair image: [slot][three RGB float4, the 4 depths]
  DynLane l[UPT];
#pragma unroll
  for (int j = 0; j < UPT; ++j) {
#pragma unroll
    for (int q = 0; q < 4; ++q) A[j][q] = D[j][q] = f32x4{0.f, 0.f, 0.f, 0.f};
    l[j] = dyn_lane<THREADS, U8>(ub, j, tid, U);
  }
  constexpr int UNR = DEPTH ? 2 : 3;      // frames in flight (the pair image's registers are not live yet in this loop)
  dyn_walk_frames<DEPTH, U8, UNR, UPT>(p, wbase, n, l, A, [] {});
  dyn_last_frame<DEPTH, U8, THREADS, UPT>(p, wbase, n, tid, l, A, D);
  // ---- per-sample min / max of both images --------------------------------------------------------------------------
  float mn1 = INFINITY, mx1 = -INFINITY, mn2 = INFINITY, mx2 = -INFINITY;
#pragma unroll
  for (int j = 0; j < UPT; ++j) dyn_lane_minmax<DEPTH>(l[j], A[j], D[j], mn1, mx1, mn2, mx2);
  __shared__ float red[NW][4];
  __shared__ float s_norm[4];      // min1, range1, min2, range2
  mn1 = wave_reduce_min(mn1); mx1 = wave_reduce_max(mx1);
  mn2 = wave_reduce_min(mn2); mx2 = wave_reduce_max(mx2);
  const int wid = tid >> 6;
  if ((tid & 63) == 0) {
    red[wid][0] = mn1; red[wid][1] = mx1; red[wid][2] = mn2; red[wid][3] = mx2;
  }
  __syncthreads();
  if (wid == 0) {
    // wave 0: lane 0 publishes and carries the count it got from its own add into the wait
    DynCtl* c = ctl + n;
    f32x4* slots = reinterpret_cast<f32x4*>(ctl + p.N) + (long long)n * bps;
    unsigned got = 0;
    if (tid == 0) got = dyn_publish_arrive<NW>(c, slots, b, red, mn1, mx1, mn2, mx2);
    dyn_collect(c, slots, got, bps, polls, tid, s_norm);
  }
  __syncthreads();
  const float m1 = s_norm[0], r1 = s_norm[1], m2 = s_norm[2], r2 = s_norm[3];
  // ---- normalise in registers, store once ---------------------------------------------------------------------------------
#pragma unroll
  for (int j = 0; j < UPT; ++j) {
    dyn_emit<DEPTH, U8, THREADS>(A[j], m1, r1, p.out, p, n, tid, l[j]);
    dyn_emit<DEPTH, U8, THREADS>(D[j], m2, r2, p.diff_out, p, n, tid, l[j]);
  }
}

// ------------------------------------------------------------------------------------------------------------------
// The same stage with TWO samples per block, one after the other (round 5, second form): with one sample per block every
// block of the chip reads for ~85 us and then stores for ~20 us, all in step -- the 100 MB of stores never overlap the 430 MB
// of loads.  Here a group of bps consecutive blocks owns samples pi and pi + half; a block runs the frame loop of its chunk of
// sample pi, publishes its min / max, and normalises + stores that sample's images from INSIDE the frame loop of sample
// pi + half (half-way through: every block of the group has long finished the first sample), so the first half of the stores
// rides beside the second half of the loads.  One unit (4 pixels) per thread and sample; everything else as above.
// ------------------------------------------------------------------------------------------------------------------
template <bool DEPTH, bool U8, int THREADS>
__global__ __launch_bounds__(THREADS) void dynimg_goal_onepass2_kernel(const DynParams p, DynCtl* ctl, int bps, int half, unsigned polls) {
  constexpr int NW = THREADS / 64;
  const int pi = blockIdx.x / bps, b = blockIdx.x - pi * bps;
  const int tid = threadIdx.x, wid = tid >> 6;
  const DynLane l[1] = {dyn_lane<THREADS, U8>((long long)b * THREADS, 0, tid, p.HW >> 2)};
  __shared__ float red[NW][4];
  __shared__ float s_norm[4];
  // ---- frame loop + last frame of sample n: A = buffer image, D = pair image (flat layout for fp32 sources); `mid()` is called
  // once, about half-way through the frames
  auto accumulate = [&](int n, f32x4 (&A)[1][4], f32x4 (&D)[1][4], auto&& mid) {
    [[maybe_unused]] const unsigned char* wbase = U8 ? p.win[n] : nullptr;
#pragma unroll
    for (int q = 0; q < 4; ++q) A[0][q] = D[0][q] = f32x4{0.f, 0.f, 0.f, 0.f};
    constexpr int UNR = DEPTH ? 3 : 4;      // frames in flight: 12 loads of 16 B per lane (the first sample's images stay live meanwhile)
    dyn_walk_frames<DEPTH, U8, UNR, 1>(p, wbase, n, l, A, mid);
    dyn_last_frame<DEPTH, U8, THREADS, 1>(p, wbase, n, tid, l, A, D);
  };
  // ---- block min / max of sample n -> its slot; count the block in
  auto publish = [&](int n, const f32x4 (&A)[1][4], const f32x4 (&D)[1][4]) {
    float mn1 = INFINITY, mx1 = -INFINITY, mn2 = INFINITY, mx2 = -INFINITY;
    dyn_lane_minmax<DEPTH>(l[0], A[0], D[0], mn1, mx1, mn2, mx2);
    mn1 = wave_reduce_min(mn1); mx1 = wave_reduce_max(mx1);
    mn2 = wave_reduce_min(mn2); mx2 = wave_reduce_max(mx2);
    __syncthreads();                     // (red may still be read by the previous sample's publish)
    if ((tid & 63) == 0) {
      red[wid][0] = mn1; red[wid][1] = mx1; red[wid][2] = mn2; red[wid][3] = mx2;
    }
    __syncthreads();
    // (the count is not carried: the wait comes later, from inside the next sample's frame loop, and reads the counter itself)
    if (tid == 0) dyn_publish_arrive<NW>(ctl + n, reinterpret_cast<f32x4*>(ctl + p.N) + (long long)n * bps, b, red, mn1, mx1, mn2, mx2);
  };
  // ---- wait for sample n's blocks, fold their slots, normalise this block's part in registers and store it
  auto finish = [&](int n, f32x4 (&A)[1][4], f32x4 (&D)[1][4]) {
    __syncthreads();                     // (s_norm may still be read by the previous sample's finish)
    if (wid == 0) {
      DynCtl* c = ctl + n;
      unsigned got = 0;
      if (tid == 0) got = __hip_atomic_load(&c->arrive, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      dyn_collect(c, reinterpret_cast<const f32x4*>(ctl + p.N) + (long long)n * bps, got, bps, polls, tid, s_norm);
    }
    __syncthreads();
    dyn_emit<DEPTH, U8, THREADS>(A[0], s_norm[0], s_norm[1], p.out, p, n, tid, l[0]);
    dyn_emit<DEPTH, U8, THREADS>(D[0], s_norm[2], s_norm[3], p.diff_out, p, n, tid, l[0]);
  };
  const int nA = pi, nB = pi + half;
  f32x4 AA[1][4], DA[1][4];
  accumulate(nA, AA, DA, [] {});
  publish(nA, AA, DA);
  if (nB < p.N) {
    f32x4 AB[1][4], DB[1][4];
    accumulate(nB, AB, DB, [&] { finish(nA, AA, DA); });
    publish(nB, AB, DB);
    finish(nB, AB, DB);
  } else {
    finish(nA, AA, DA);
  }
}

// The goal model's three conv1 inputs (graph.py:386-401) in ONE launch (round 5; round 4: two, round 3: three, before: five):
// one pass over the window computes the buffer image and the pair image of (current frame, target) in registers, writes the
// current frame's padded copy, and normalises both images before their only store (dynimg_goal_onepass_kernel).
// ws = geeco_goal_dynimgs_ws_bytes(N, HW) bytes, ZERO-FILLED once by the caller; every call leaves its counters zero.
extern "C" int64_t geeco_goal_dynimgs_ws_bytes(int N, int64_t HW) {
  if (N <= 0 || HW <= 0) return 0;
  return (int64_t)N * ((int64_t)sizeof(DynCtl) + cdiv64(HW >> 2, 256) * 16);      // counters + the most slots a sample can have
}

// Blocks whose wait for the other blocks of their sample has EVER expired on this workspace, summed over the N samples (sticky
// until the caller zero-fills ws again; such samples' images are NaN, see above).  0 = every image that came out of this
// workspace was normalised with its sample's true min / max.  Copies N x 64 bytes to the host and SYNCHRONISES the stream: for
// the places where the host waits for the device anyway (loss read-out, end of an epoch), not for the step.
extern "C" int geeco_goal_dynimgs_timeouts(const void* ws, int N, void* stream, int64_t* count_host) {
  GEECO_CHECK_ARG(ws && count_host && N >= 1, "goal_dynimgs_timeouts: null pointer / N=%d", N);
  std::vector<DynCtl> host((size_t)N);
  hipStream_t s = (hipStream_t)stream;
  hipError_t e = hipMemcpyAsync(host.data(), ws, (size_t)N * sizeof(DynCtl), hipMemcpyDeviceToHost, s);
  if (e == hipSuccess) e = hipStreamSynchronize(s);
  if (e != hipSuccess) {
    geeco_set_error("goal_dynimgs_timeouts: %s", hipGetErrorString(e));
    return (int)e;
  }
  int64_t n = 0;
  for (const DynCtl& c : host) n += c.timeouts;
  *count_host = n;
  return 0;
}

// Polls a block spends waiting for its sample's blocks before it reports a timeout (process-wide; default 2^22, i.e. seconds).
// Returns the previous value.  0 makes every block that is not the last of its sample to arrive report at once: how the tests
// provoke the error path deterministically.
extern "C" unsigned geeco_goal_dynimgs_set_wait_polls(unsigned polls) {
  const unsigned old = g_wait_polls;
  g_wait_polls = polls;
  return old;
}

template <bool DEPTH, bool U8>
static void goal_onepass_dispatch(const DynParams& p, DynCtl* ctl, hipStream_t s) {
  const long long U = p.HW >> 2;
  // 1024-thread blocks of 2 units per thread (8 pixels: 48 / 64 accumulator registers of both images) when that still gives
  // the chip about a block per CU; otherwise 256-thread blocks of one unit (small batches: the predictor's N = 1)
  const long long bps_big = cdiv64(U, 2048);
  if ((long long)p.N * bps_big >= 192) {
    if constexpr (!U8) {
      // fp32 windows: two samples per block, the first one's stores inside the second one's frame loop (same box, in the step:
      // 105.7-108.0 us against 110.9-114.7 for one sample per block)
      const int half = (p.N + 1) / 2, bps2 = (int)cdiv64(U, 1024);
      geeco_note_kernel("dynimg_goal_onepass2_kernel<%s, %s, 1024>", DEPTH ? "true" : "false", U8 ? "true" : "false");
      hipLaunchKernelGGL((dynimg_goal_onepass2_kernel<DEPTH, U8, 1024>), dim3((unsigned)(half * bps2)), dim3(1024), 0, s, p, ctl, bps2, half, g_wait_polls);
    } else {
      // uint8 frames: a quarter of the bytes and twelve conversions per pixel: the load phase is short and the one-sample form
      // with two units per thread keeps more of it in flight (58.6 us alone against 63.8)
      geeco_note_kernel("dynimg_goal_onepass_kernel<%s, %s, 1024, 2>", DEPTH ? "true" : "false", U8 ? "true" : "false");
      hipLaunchKernelGGL((dynimg_goal_onepass_kernel<DEPTH, U8, 1024, 2>), dim3((unsigned)(p.N * bps_big)), dim3(1024), 0, s, p, ctl, (int)bps_big, g_wait_polls);
    }
  } else {
    const long long bps = cdiv64(U, 256);
    geeco_note_kernel("dynimg_goal_onepass_kernel<%s, %s, 256, 1>", DEPTH ? "true" : "false", U8 ? "true" : "false");
    hipLaunchKernelGGL((dynimg_goal_onepass_kernel<DEPTH, U8, 256, 1>), dim3((unsigned)(p.N * bps)), dim3(256), 0, s, p, ctl, (int)bps, g_wait_polls);
  }
}

static int goal_dynimgs_launch(DynParams& p, const float* alpha_host, const float* alpha2_host, bool u8, float* cur_out,
                               float* buf_out, float* diff_out, void* ws, void* stream) {
  hipStream_t s = (hipStream_t)stream;
  GEECO_CHECK_ARG((long long)p.N * cdiv64(p.HW >> 2, 256) < (1ll << 31) && p.HW * 16 < (1ll << 31),
                  "goal_dynimgs: %d samples of %lld pixels exceed the grid / the 32-bit in-frame offsets", p.N, p.HW);
  p.C = 3; p.Cpad = 4; p.out = buf_out; p.last = cur_out;
  for (int t = 0; t < p.K; ++t) p.alpha[t] = alpha_host[t];
  p.diff_out = diff_out;
  p.alpha2[0] = alpha2_host[0]; p.alpha2[1] = alpha2_host[1];
  DynCtl* ctl = (DynCtl*)ws;
  const bool depth = p.depth != nullptr;
  if (u8) {
    if (depth) goal_onepass_dispatch<true, true>(p, ctl, s);
    else goal_onepass_dispatch<false, true>(p, ctl, s);
  } else {
    if (depth) goal_onepass_dispatch<true, false>(p, ctl, s);
    else goal_onepass_dispatch<false, false>(p, ctl, s);
  }
  GEECO_LAUNCH_CHECK();
  return 0;
}

extern "C" int geeco_goal_dynimgs_fwd(const float* rgb, int64_t sample_stride, int64_t frame_stride, const float* tgt_rgb,
                                      const float* depth, int64_t dsample_stride, int64_t dframe_stride,
                                      const float* tgt_depth, const float* alpha_host, const float* alpha2_host, int N, int K,
                                      int64_t HW, float* cur_out, float* buf_out, float* diff_out, void* ws, void* stream) {
  GEECO_CHECK_ARG(rgb && tgt_rgb && alpha_host && alpha2_host && cur_out && buf_out && diff_out && ws,
                  "goal_dynimgs_fwd: null pointer");
  GEECO_CHECK_ARG((!depth) == (!tgt_depth), "goal_dynimgs_fwd: depth and tgt_depth come together");
  GEECO_CHECK_ARG(K >= 1 && K <= DYN_MAXK, "goal_dynimgs_fwd: K=%d outside 1..%d", K, DYN_MAXK);
  GEECO_CHECK_ARG(N >= 1 && HW >= 4 && (HW & 3) == 0, "goal_dynimgs_fwd: HW=%lld must be a multiple of 4", (long long)HW);
  GEECO_CHECK_ARG(sample_stride % 4 == 0 && frame_stride % 4 == 0 && dsample_stride % 4 == 0 && dframe_stride % 4 == 0,
                  "goal_dynimgs_fwd: 16-byte aligned frames");
  DynParams p = {};
  p.frames = rgb; p.sample_stride = sample_stride; p.frame_stride = frame_stride;
  p.depth = depth; p.dsample_stride = dsample_stride; p.dframe_stride = dframe_stride;
  p.N = N; p.K = K; p.HW = HW;
  p.tgt = tgt_rgb; p.tgt_depth = tgt_depth;
  return goal_dynimgs_launch(p, alpha_host, alpha2_host, false, cur_out, buf_out, diff_out, ws, stream);
}

// The same input stage fed from the episodes' resident uint8 frames (the data path's "next" row: the window of
// _window_v3, geeco_gym.py:615-631, and the / 255 of _parse_v4, :312, happen inside the load): win_ptrs_dev / tgt_ptrs_dev are
// DEVICE arrays of N addresses (window n = K consecutive [HW][3] uint8 frames starting at win_ptrs_dev[n]; its target frame
// at tgt_ptrs_dev[n]), so a captured graph keeps replaying while the host repoints the tables between steps.  Depth (float32)
// stays a dense [N][K][HW] / [N][HW] tensor.  Outputs are bitwise those of geeco_gather_windows + geeco_goal_dynimgs_fwd.
extern "C" int geeco_goal_dynimgs_u8_fwd(const void* const* win_ptrs_dev, const void* const* tgt_ptrs_dev, const float* depth,
                                         int64_t dsample_stride, int64_t dframe_stride, const float* tgt_depth,
                                         const float* alpha_host, const float* alpha2_host, int N, int K, int64_t HW,
                                         float* cur_out, float* buf_out, float* diff_out, void* ws, void* stream) {
  GEECO_CHECK_ARG(win_ptrs_dev && tgt_ptrs_dev && alpha_host && alpha2_host && cur_out && buf_out && diff_out && ws,
                  "goal_dynimgs_u8_fwd: null pointer");
  GEECO_CHECK_ARG((!depth) == (!tgt_depth), "goal_dynimgs_u8_fwd: depth and tgt_depth come together");
  GEECO_CHECK_ARG(K >= 1 && K <= DYN_MAXK, "goal_dynimgs_u8_fwd: K=%d outside 1..%d", K, DYN_MAXK);
  GEECO_CHECK_ARG(N >= 1 && HW >= 4 && (HW & 3) == 0, "goal_dynimgs_u8_fwd: HW=%lld must be a multiple of 4", (long long)HW);
  GEECO_CHECK_ARG(dsample_stride % 4 == 0 && dframe_stride % 4 == 0, "goal_dynimgs_u8_fwd: 16-byte aligned depth frames");
  DynParams p = {};
  p.win = reinterpret_cast<const unsigned char* const*>(win_ptrs_dev);
  p.tgt_u8 = reinterpret_cast<const unsigned char* const*>(tgt_ptrs_dev);
  p.depth = depth; p.dsample_stride = dsample_stride; p.dframe_stride = dframe_stride;
  p.N = N; p.K = K; p.HW = HW;
  p.tgt_depth = tgt_depth;
  return goal_dynimgs_launch(p, alpha_host, alpha2_host, true, cur_out, buf_out, diff_out, ws, stream);
}
