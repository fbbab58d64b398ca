// hd.h - HLMI_HD: what stands in front of a function that the kernels and a plain host translation unit both compile (dec_text.h,
// row_score.h, sr_overlaps.h, polish_rows.h and their checks under tests/capi/).  A host compiler sees nothing of HIP's here.
#pragma once

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define HLMI_HD __host__ __device__ __forceinline__
#else
#define HLMI_HD inline
#endif
