// The colour byte of the mesh export, written once: the vertex record of mesh_attr.hip (include/oi_mesh_attr.h) and the
// byte atlases of mesh_tex.hip (include/oi_mesh_tex.h) hold round-to-nearest-even of clamp(c, 0, 1) * 255, NaN -> 0.
#pragma once
#include <hip/hip_runtime.h>

namespace oi {

__device__ __forceinline__ unsigned char quant8(float c) {
  return (unsigned char)__float2int_rn(fminf(fmaxf(c, 0.f), 1.f) * 255.f);  // fmaxf(NaN, 0) = 0
}

}  // namespace oi
