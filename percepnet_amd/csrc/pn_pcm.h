// float -> int16 PCM, shared by the back end's fused cast (pn_dsp.hip), the output stage (pn_outstage.hip) and the rate
// converter's down kernel (pn_rate.hip).
#pragma once
#include "pn_common.h"

// float -> int16 as the reference CLI's x86-64 build does it (main.cpp:36): truncate toward zero
// to int32 (cvttss2si; NaN / out of range -> 0x80000000), keep the low 16 bits.
__device__ __forceinline__ int16_t pn_f2s(float v) {
  const int32_t t = (fabsf(v) < 2147483648.f) ? (int32_t)v : (int32_t)0x80000000;
  return (int16_t)(uint16_t)((uint32_t)t & 0xffffu);
}

// the saturating cast of t = o * 32768: NaN -> 0, else trunc(t) clamped to the int16 range
__device__ __forceinline__ int16_t pn_f2s_sat(float t) {
  if (t >= 32768.f) return 32767;
  if (t <= -32769.f) return -32768;
  return t == t ? (int16_t)(int32_t)t : (int16_t)0;
}
