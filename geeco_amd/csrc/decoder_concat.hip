// =====================================================================================================
// state concat (graph.py:138-141, 162-165, 187-190)
// =====================================================================================================
#include "decoder_internal.h"

__global__ __launch_bounds__(256) void concat_fwd_kernel(const ConcatParams p) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  const long long per = (long long)p.cells * p.Ctot;
  if (i >= per * p.N) return;
  const int n = (int)(i / per);
  const int rem = (int)(i - (long long)n * per);
  const int cell = rem / p.Ctot, c = rem - cell * p.Ctot;
  float v;
  if (c >= p.jnt_off && c < p.jnt_off + p.J) {
    v = p.jnt[(long long)n * p.jnt_stride + (c - p.jnt_off)];
  } else {
    int f = 0;
#pragma unroll
    for (int k = 1; k < 3; ++k)
      if (k < p.nfeat && c >= p.off[k]) f = k;
    const int cc = c - p.off[f];
    const long long idx = ((long long)n * p.cells + cell) * p.ch[f] + cc;
    v = p.feats[f][idx];
    if (f == 0 && p.sub_from) v = p.sub_from[idx] - v;
  }
  p.state[(long long)n * p.state_stride + rem] = v;
}

// blockIdx.y = feature map (all of them in one launch; maps without a gradient buffer are skipped)
__global__ __launch_bounds__(256) void concat_bwd_kernel(const ConcatParams p) {
  const int f = blockIdx.y;
  if (!p.dfeats[f]) return;
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  const long long per = (long long)p.cells * p.ch[f];
  if (i >= per * p.N) return;
  const int n = (int)(i / per);
  const int rem = (int)(i - (long long)n * per);
  const int cell = rem / p.ch[f], c = rem - cell * p.ch[f];
  float d = p.state[(long long)n * p.state_stride + cell * p.Ctot + p.off[f] + c];
  d = p.feats[f][i] > 0.f ? d * p.scale : 0.f;      // ReluGrad of the encoder's last layer
  p.dfeats[f][i] = p.accumulate ? p.dfeats[f][i] + d : d;
}

// (the general form; state_layout.h holds its three-mode special case for the window kernels)
int fill_concat(ConcatParams* p, const int* feat_ch, int nfeat, int jnt_pos, int J) {
  int off = 0;
  for (int i = 0; i < nfeat; ++i) {
    if (i == jnt_pos) {
      p->jnt_off = off;
      off += J;
    }
    p->ch[i] = feat_ch[i];
    p->off[i] = off;
    off += feat_ch[i];
  }
  if (jnt_pos >= nfeat) {
    p->jnt_off = off;
    off += J;
  }
  p->Ctot = off;
  p->nfeat = nfeat;
  p->J = J;
  return off;
}

extern "C" int geeco_state_concat_fwd(const float* const* feats, const int* feat_ch, int nfeat, int jnt_pos,
                                      const float* jnt, int64_t jnt_stride, int J, const float* sub_from, int N,
                                      int cells, float* state, int64_t state_stride, void* stream) {
  GEECO_CHECK_ARG(feats && feat_ch && jnt && state, "state_concat_fwd: null pointer");
  GEECO_CHECK_ARG(nfeat >= 1 && nfeat <= 3 && jnt_pos >= 0 && jnt_pos <= nfeat, "state_concat_fwd: nfeat/jnt_pos");
  ConcatParams p = {};
  fill_concat(&p, feat_ch, nfeat, jnt_pos, J);
  for (int i = 0; i < nfeat; ++i) p.feats[i] = feats[i];
  p.jnt = jnt; p.jnt_stride = jnt_stride; p.sub_from = sub_from; p.N = N; p.cells = cells;
  p.state = state; p.state_stride = state_stride;
  GEECO_CHECK_ARG(state_stride >= (int64_t)cells * p.Ctot, "state_concat_fwd: state_stride too small");
  const long long total = (long long)N * cells * p.Ctot;
  hipLaunchKernelGGL(concat_fwd_kernel, dim3((unsigned)cdiv64(total, 256)), dim3(256), 0, (hipStream_t)stream, p);
  GEECO_LAUNCH_CHECK();
  return 0;
}

extern "C" int geeco_state_concat_bwd(const float* dstate, int64_t dstate_stride, const float* const* feats_fwd,
                                      float* const* dfeats, const int* feat_ch, int nfeat, int jnt_pos, int J, int N,
                                      int cells, int accumulate, float scale, void* stream) {
  GEECO_CHECK_ARG(dstate && feats_fwd && dfeats && feat_ch, "state_concat_bwd: null pointer");
  GEECO_CHECK_ARG(nfeat >= 1 && nfeat <= 3 && jnt_pos >= 0 && jnt_pos <= nfeat, "state_concat_bwd: nfeat/jnt_pos");
  ConcatParams p = {};
  fill_concat(&p, feat_ch, nfeat, jnt_pos, J);
  p.state = const_cast<float*>(dstate); p.state_stride = dstate_stride; p.N = N; p.cells = cells;
  p.accumulate = accumulate;
  p.scale = scale;
  for (int i = 0; i < nfeat; ++i) {
    p.feats[i] = feats_fwd[i];
    p.dfeats[i] = dfeats[i];
  }
  long long most = 0;
  for (int f = 0; f < nfeat; ++f) {
    if (!dfeats[f]) continue;
    GEECO_CHECK_ARG(feats_fwd[f], "state_concat_bwd: feats_fwd[%d] is null", f);
    const long long total = (long long)N * cells * p.ch[f];
    if (total > most) most = total;
  }
  if (most == 0) return 0;
  hipLaunchKernelGGL(concat_bwd_kernel, dim3((unsigned)cdiv64(most, 256), (unsigned)nfeat), dim3(256), 0,
                     (hipStream_t)stream, p);
  GEECO_LAUNCH_CHECK();
  return 0;
}
