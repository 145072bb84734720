// Device leaf helpers shared by the scoring kernels (scoring.hip, search.hip, plda.hip, snorm.hip): the 4-float vector type, the
// guarded fragment load, the wavefront synchronisation of LDS data private to one wave and the score normalisation's
// expression.  Leaf code only: the three tiled product loops (cosine_tiled_kernel, search_tiles_kernel, plda_product_kernel),
// their staging, K order and epilogues stay in their kernels.  The two trial-list kernels (pair_scores_kernel, plda_pair_kernel) and backend.hip's load_quad keep their own
// statements: written as shared helpers they compile to other instruction streams.
#pragma once
#include <hip/hip_runtime.h>

typedef float f32x4 __attribute__((ext_vector_type(4)));

namespace {

// Floats [col, col + 4) of a row as an MFMA fragment: zeros for a row outside its matrix and past dim; one 16-byte load where
// the quad lies inside the row and vec_ok (dim % 4 == 0, 16-byte aligned matrix), guarded 4-byte loads otherwise.
__device__ __forceinline__ f32x4 load4(const float* row, int col, int dim, bool row_ok, bool vec_ok) {
  f32x4 v = (f32x4){0.f, 0.f, 0.f, 0.f};
  if (!row_ok) return v;
  if (vec_ok && col + 4 <= dim) return *reinterpret_cast<const f32x4*>(row + col);
#pragma unroll
  for (int e = 0; e < 4; ++e)
    if (col + e < dim) v[e] = row[col + e];
  return v;
}

// One wave's DS instructions execute in order; this keeps the compiler from moving a lane's LDS accesses across the point
// where another lane's become visible to it.
__device__ __forceinline__ void wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// One normalised score, svk_score_norm's expression (svk.h "score normalisation"; svk_cosine_topk_norm ranks by the same bits):
// float64 throughout, every operation rounded on its own, in the order written.  r: the row (test, T-norm) side's moments,
// c: the column (enrolled, Z-norm) side's.  Nothing is clamped: a zero, negative or NaN sd gives what IEEE arithmetic gives.
__device__ __forceinline__ float norm_value(float s, bool has_r, double mu_r, double sd_r, bool has_c, double mu_c, double sd_c) {
#pragma clang fp contract(off)
  const double x = (double)s;
  if (has_r && has_c) return (float)(0.5 * ((x - mu_r) / sd_r + (x - mu_c) / sd_c));
  return (float)(has_r ? (x - mu_r) / sd_r : (x - mu_c) / sd_c);
}

}  // namespace
