// rs_build.h -- the tree builders' internal header: the entry points that rs_bvh_build.hip and rs_wide_build.hip
// define and that restir_capi.hip and each other call, and the ordered-int float pair of their min / max atomics.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string>
#include <vector>
#include "rs_refit.h"

namespace rs {

// ---- rs_bvh_build.hip
// The scene's trees for the n triangles at d_pos (n * 9 floats, device): the binary skip-pointer tree (*d_nodes:
// 2 float4 per node plus one zeroed pad node, *d_tris: 3 float4 per triangle; new device allocations owned by the
// caller; PLOC, or the LBVH under RESTIR_BVH=lbvh) and, with `wide`, the optional 8-wide tree (wide->status says why
// there is none).  0, or -1 with err set.
int build_bvh(const float* d_pos, uint32_t n, hipStream_t st, float4** d_nodes, uint32_t* n_nodes, float4** d_tris,
              WideBvh* wide, std::string& err);
int build_bvh_lbvh(const float* d_pos, uint32_t n, hipStream_t st, float4** d_nodes, uint32_t* n_nodes,
                   float4** d_tris, std::string& err);
int build_bvh_ploc(const float* d_pos, uint32_t n, hipStream_t st, float4** d_nodes, uint32_t* n_nodes,
                   float4** d_tris, std::string& err);
void preload_code_objects();
void wide_free(WideBvh& w);
// stream-ordered scratch from the builders' private pool; builder_pool_trim returns it to the driver after a build
hipError_t pool_malloc(void** p, size_t bytes, hipStream_t st);
void builder_pool_trim();
int bvh_refit_plan(const float4* d_nodes, uint32_t n_nodes, hipStream_t st, int** d_order, int** d_lvl_off,
                   std::vector<int>& lvl_off, std::string& err);
int bvh_refit(float4* d_nodes, float4* d_tris, const float* d_pos, const int* d_order, const int* d_lvl_off,
              const std::vector<int>& lvl_off, hipStream_t st, int* tail, std::string& err);
// ---- rs_wide_build.hip
int build_wide_gpu(const float* d_pos, int n, hipStream_t st, WideBvh* w, std::string& err);
void preload_wide_build();

// order-preserving float <-> int, for min / max of floats by integer atomics
__device__ __forceinline__ int f2o(float f) {
    const int i = __float_as_int(f);
    return i >= 0 ? i : i ^ 0x7fffffff;
}
__device__ __forceinline__ float o2f(int i) { return __int_as_float(i >= 0 ? i : i ^ 0x7fffffff); }

}  // namespace rs
