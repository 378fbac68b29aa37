// Internal helpers shared by the gfx950 kernels of libtavsr_hip.so.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "tavsr.h"

namespace tavsr {

void set_error(const char* fmt, ...);

#define TAVSR_REQUIRE(cond, code, ...)   \
  do {                                   \
    if (!(cond)) {                       \
      ::tavsr::set_error(__VA_ARGS__);   \
      return (code);                     \
    }                                    \
  } while (0)

// Launch-status check: never synchronises (graph-capture safe).
#define TAVSR_LAUNCH_CHECK()                                                   \
  do {                                                                         \
    hipError_t e__ = hipGetLastError();                                        \
    if (e__ != hipSuccess) {                                                   \
      ::tavsr::set_error("%s:%d launch failed: %s", __FILE__, __LINE__,        \
                         hipGetErrorString(e__));                              \
      return (int)e__;                                                         \
    }                                                                          \
  } while (0)

constexpr int kWave = 64;

// The lane-network reductions below use the row_bcast:15 / row_bcast:31 DPP controls, which exist on GFX9 / CDNA only, and this
// library is written for one ISA.  A device pass for anything else stops here instead of assembling garbage.
#if defined(__HIP_DEVICE_COMPILE__) && !defined(__gfx950__)
#error "libtavsr_hip kernels are written for gfx950 (CDNA4): build with --offload-arch=gfx950"
#endif
// Debug builds (-DTAVSR_DEBUG_WAVE) trap when a whole-wave reduction is entered with lanes switched off: the result is read from
// lane 63 and the row broadcasts take their sources by lane number, so a partial wave would return a stale value silently.
#ifdef TAVSR_DEBUG_WAVE
#define TAVSR_ASSERT_FULL_WAVE() do { if (__builtin_amdgcn_read_exec() != ~0ull) __builtin_trap(); } while (0)
#else
#define TAVSR_ASSERT_FULL_WAVE() do { } while (0)
#endif

// Whole-wave reductions on the data-parallel-primitive lane network (quad permutes, row mirrors, row broadcasts; the result is read
// from lane 63 and is uniform): six steps of ~8 cycles against six dependent ds_bpermute round trips (~120 cycles each) of a
// __shfl_xor butterfly.  LayerNorm rows, softmax rows and the selection loops of the search step are chains of such reductions.
// All 64 lanes must be active (every caller reduces under wave-uniform control flow).  `IDENT`: what a lane that a step does
// not write contributes (0 for sums; the lane's own value for max / min).
#define TAVSR_DPP_F(V, CTRL, RMASK, OLD) __int_as_float(__builtin_amdgcn_update_dpp(__float_as_int(OLD), __float_as_int(V), CTRL, RMASK, 0xf, false))
__device__ __forceinline__ float wave_sum(float v) {
  TAVSR_ASSERT_FULL_WAVE();
  v += TAVSR_DPP_F(v, 0xB1, 0xf, 0.f);       // quad_perm [1, 0, 3, 2]
  v += TAVSR_DPP_F(v, 0x4E, 0xf, 0.f);       // quad_perm [2, 3, 0, 1]
  v += TAVSR_DPP_F(v, 0x141, 0xf, 0.f);      // row_half_mirror
  v += TAVSR_DPP_F(v, 0x140, 0xf, 0.f);      // row_mirror: every lane of a row of 16 holds the row's sum
  v += TAVSR_DPP_F(v, 0x142, 0xa, 0.f);      // row_bcast:15 into rows 1 and 3
  v += TAVSR_DPP_F(v, 0x143, 0xc, 0.f);      // row_bcast:31 into rows 2 and 3
  return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 63));
}
__device__ __forceinline__ float wave_max(float v) {
  TAVSR_ASSERT_FULL_WAVE();
  v = fmaxf(v, TAVSR_DPP_F(v, 0xB1, 0xf, v));
  v = fmaxf(v, TAVSR_DPP_F(v, 0x4E, 0xf, v));
  v = fmaxf(v, TAVSR_DPP_F(v, 0x141, 0xf, v));
  v = fmaxf(v, TAVSR_DPP_F(v, 0x140, 0xf, v));
  v = fmaxf(v, TAVSR_DPP_F(v, 0x142, 0xa, v));
  v = fmaxf(v, TAVSR_DPP_F(v, 0x143, 0xc, v));
  return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 63));
}
__device__ __forceinline__ float wave_max_dpp(float v) { return wave_max(v); }
__device__ __forceinline__ int wave_min_dpp(int v) {
  TAVSR_ASSERT_FULL_WAVE();
#define TAVSR_DPP_I(CTRL, RMASK) v = min(v, __builtin_amdgcn_update_dpp(v, v, CTRL, RMASK, 0xf, false))
  TAVSR_DPP_I(0xB1, 0xf);
  TAVSR_DPP_I(0x4E, 0xf);
  TAVSR_DPP_I(0x141, 0xf);
  TAVSR_DPP_I(0x140, 0xf);
  TAVSR_DPP_I(0x142, 0xa);
  TAVSR_DPP_I(0x143, 0xc);
#undef TAVSR_DPP_I
  return __builtin_amdgcn_readlane(v, 63);
}

// Activations on the hardware transcendentals (v_exp_f32 / v_rcp_f32, 1 ulp each) instead of libm's expf / erff and an IEEE
// division: Swish 6 instructions instead of ~35, GELU ~16 instead of ~50 (erff is two branches of ~45, both taken by a wave) -
// in a K = 256 GEMM epilogue the libm GELU cost 40 % of the tile's MFMA time, in the LayerNorm backward of cgMLP's gate half it
// was most of the launch.  erf: Abramowitz & Stegun 7.1.26, |error| <= 1.5e-7 absolute; everything here is ~1e-7 relative on the
// activation's value, three orders inside the 1e-4 parity bar (espnet: torch.nn.GELU() = erf form, Swish = x * sigmoid(x)).
__device__ __forceinline__ float sigmoid_fast(float z) {
  return __builtin_amdgcn_rcpf(1.f + __builtin_amdgcn_exp2f(-1.4426950408889634f * z));
}
// (E = exp(-x^2), shared by erf's tail and the normal density of the GELU derivative)
__device__ __forceinline__ float erf_from_exp(float x, float E) {
  const float ax = fabsf(x);
  const float t = __builtin_amdgcn_rcpf(fmaf(0.3275911f, ax, 1.f));
  float p = fmaf(1.061405429f, t, -1.453152027f);
  p = fmaf(p, t, 1.421413741f);
  p = fmaf(p, t, -0.284496736f);
  p = fmaf(p, t, 0.254829592f);
  return copysignf(fmaf(-p * t, E, 1.f), x);
}
__device__ __forceinline__ float act_fwd(int act, float z) {
  switch (act) {
    case TAVSR_ACT_RELU: return z > 0.f ? z : 0.f;
    case TAVSR_ACT_SWISH: return z * sigmoid_fast(z);
    case TAVSR_ACT_GELU: {
      const float E = __builtin_amdgcn_exp2f(-0.72134752044448170368f * z * z);      // exp(-z^2 / 2)
      return 0.5f * z * (1.f + erf_from_exp(z * 0.70710678118654752440f, E));
    }
    default: return z;
  }
}
// derivative of the activation at pre-activation z
__device__ __forceinline__ float act_bwd(int act, float z) {
  switch (act) {
    case TAVSR_ACT_RELU: return z > 0.f ? 1.f : 0.f;
    case TAVSR_ACT_SWISH: {
      const float s = sigmoid_fast(z);
      return s * (1.f + z * (1.f - s));
    }
    case TAVSR_ACT_GELU: {
      const float E = __builtin_amdgcn_exp2f(-0.72134752044448170368f * z * z);      // exp(-z^2 / 2)
      const float cdf = 0.5f * (1.f + erf_from_exp(z * 0.70710678118654752440f, E));
      return cdf + z * (0.39894228040143267794f * E);
    }
    default: return 1.f;
  }
}

// tanh, hardtanh and SELU (TAVSR_ACT_TANH ..): the rest of espnet get_activation's set, for the encoders' feed-forward blocks.
// NOT cases of act_fwd / act_bwd above: a wider run-time switch costs registers (and occupancy) in every kernel that takes the
// activation at run time; these are instantiated where they are used (the streaming FFN kernels' template argument, the GEMM's
// stand-alone epilogue for them).  Same hardware transcendentals.  Near 0 the closed forms cancel (1 - 2 / (e^2z + 1) and
// e^z - 1 keep ~4 significant digits at |z| = 1e-3), so |z| < 1/4 takes short Taylor series instead (truncation < 1e-8
// relative); above that the cancellation costs at most 2 bits.  tanh' = r (2 - r) with r = 1 - tanh|z| = 2 / (e^2|z| + 1) has
// no cancellation where tanh saturates.  Derivatives at the kinks as torch autograd takes them: hardtanh' = 0 at |z| >= 1,
// selu'(0) = scale * alpha (elu_backward: the negative branch at z <= 0).
constexpr float kSeluScale = 1.0507009873554805f, kSeluAlpha = 1.6732632423543772f;
__device__ __forceinline__ float tanh_small(float z) {      // |z| < 1/4: z - z^3/3 + 2z^5/15 - 17z^7/315 + 62z^9/2835
  const float z2 = z * z;
  return fmaf(z * z2, fmaf(z2, fmaf(z2, fmaf(z2, 0.021869488536155203f, -0.053968253968253971f), 0.13333333333333333f),
                           -0.33333333333333333f), z);
}
__device__ __forceinline__ float tanh_rest(float az) {      // 1 - tanh|z|
  return 2.f * __builtin_amdgcn_rcpf(1.f + __builtin_amdgcn_exp2f(2.8853900817779268f * az));
}
__device__ __forceinline__ float tanh_fast(float z) {
  const float az = fabsf(z);
  return az < 0.25f ? tanh_small(z) : copysignf(1.f - tanh_rest(az), z);
}
__device__ __forceinline__ float dtanh_fast(float z) {
  const float az = fabsf(z);
  if (az < 0.25f) {
    const float t = tanh_small(z);
    return fmaf(-t, t, 1.f);
  }
  const float r = tanh_rest(az);
  return r * (2.f - r);
}
__device__ __forceinline__ float hardtanh_fwd(float z) { return z < -1.f ? -1.f : (z > 1.f ? 1.f : z); }
__device__ __forceinline__ float hardtanh_bwd(float z) { return (z <= -1.f || z >= 1.f) ? 0.f : 1.f; }
__device__ __forceinline__ float selu_fast(float z) {
  if (z > 0.f) return kSeluScale * z;
  const float em1 = z > -0.25f      // e^z - 1
      ? z * fmaf(z, fmaf(z, fmaf(z, fmaf(z, fmaf(z, fmaf(z, 1.9841269841269841e-4f, 1.3888888888888889e-3f),
                                                      8.3333333333333333e-3f), 4.1666666666666667e-2f), 0.16666666666666667f),
                         0.5f), 1.f)
      : __builtin_amdgcn_exp2f(1.4426950408889634f * z) - 1.f;
  return (kSeluScale * kSeluAlpha) * em1;
}
__device__ __forceinline__ float dselu_fast(float z) {
  return z <= 0.f ? (kSeluScale * kSeluAlpha) * __builtin_amdgcn_exp2f(1.4426950408889634f * z) : kSeluScale;
}
inline bool act_is_ext(int act) { return act == TAVSR_ACT_TANH || act == TAVSR_ACT_HARDTANH || act == TAVSR_ACT_SELU; }
// kernels with the run-time switch above take these codes only (the library refuses the others there: nothing is launched)
inline bool act_base_ok(int act) { return act >= TAVSR_ACT_NONE && act <= TAVSR_ACT_GELU; }
// every code: for the kernels instantiated for the new ones
__device__ __forceinline__ float act_fwd_all(int act, float z) {
  switch (act) {
    case TAVSR_ACT_TANH: return tanh_fast(z);
    case TAVSR_ACT_HARDTANH: return hardtanh_fwd(z);
    case TAVSR_ACT_SELU: return selu_fast(z);
    default: return act_fwd(act, z);
  }
}
__device__ __forceinline__ float act_bwd_all(int act, float z) {
  switch (act) {
    case TAVSR_ACT_TANH: return dtanh_fast(z);
    case TAVSR_ACT_HARDTANH: return hardtanh_bwd(z);
    case TAVSR_ACT_SELU: return dselu_fast(z);
    default: return act_bwd(act, z);
  }
}

// Philox4x32-10 counter-based generator (dropout masks, bootstrap resampling)
__device__ __forceinline__ void philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1,
                                              uint32_t (&out)[4]) {
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
    const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
    c1 = (uint32_t)p1; c3 = (uint32_t)p0; c0 = n0; c2 = n2;
    k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
  }
  out[0] = c0; out[1] = c1; out[2] = c2; out[3] = c3;
}

int probe_fork(hipStream_t forked, hipStream_t caller, bool at_join);   // probe.hip: race amplifier at C-side forks / joins

inline int cdiv(long a, long b) { return (int)((a + b - 1) / b); }

// dwconv_time.hip: the summed partial slab [C][K+1] of a depthwise convolution's backward -> dw [C][K] and dbias [C] (tap K is the
// bias); shared by the core's three forms and by tavsr_dwconv_gate_bwd's K = 31 kernel (cgmlp.hip)
int dwconv_split(const float* sum, float* dw, float* dbias, int C, int K, int accumulate, hipStream_t stream);

// dwconv_time.hip: its gate form, out = r * (bias + dwconv_K(gn)), behind tavsr_dwconv_gate_fwd / _bwd (cgmlp.hip) at K != 31.  Odd
// K <= 63; an empty shape (B, T or C <= 0) launches nothing; a kernel size or a shape the core does not index: TAVSR_EUNSUPPORTED.
// dt_bwd_ws: floats of workspace of the core's backward, any form
int dt_gate_fwd(const float* gn, const float* r, int64_t ldr, const float* w, const float* bias, float* out, float* conv, int B, int T,
                int C, int K, tavsr_stream_t stream);
int dt_gate_bwd(const float* du, const float* gn, const float* r, int64_t ldr, const float* conv, const float* w, float* dr,
                int64_t lddr, float* dgn, float* dw, float* dbias, int accumulate, float* ws, int B, int T, int C, int K,
                tavsr_stream_t stream);
int64_t dt_bwd_ws(int32_t B, int32_t T, int32_t C, int32_t K);

}  // namespace tavsr
