// Internal declarations shared by the translation units of libsvk.so (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../../include/svk.h"

struct svk_ctx {
  int device = 0;
  hipStream_t stream = nullptr;
  int num_cu = 256;
  int clock_khz = 0;
  int lds_per_cu = 160 * 1024;
  void* scratch = nullptr;  // SVK_SCRATCH_BYTES of device memory: counters that one launch zeroes and uses (map below)
  void* work = nullptr;     // grow-only device workspace owned by the handle (row norms of svk_cosine_scores)
  size_t work_bytes = 0;
  void* comm = nullptr;     // RCCL communicator (svk_comm_init), or NULL
  int comm_ranks = 0, comm_rank = 0;
  char err[512] = {0};
};

// ctx->scratch, by byte offset.  Each slot is zeroed in stream order by the launch that uses it, so two entry points may share
// one as long as they run on the handle's stream (svk_c3d2_stage1 and svk_c3d2_stage1_c3 do).
constexpr size_t SVK_SCRATCH_BYTES = 256;
constexpr size_t SVK_SLOT_LOG_POWER = 0;       // svk_log_power: the running maximum (1 word)
constexpr size_t SVK_SLOT_STAGE2 = 64;         // svk_c3d2_stage2: its work-item counter (1 word; 2 on the two-kernel reference path)
constexpr size_t SVK_SLOT_CONV31 = 80;         // svk_c3d2_conv31 (1 word)
constexpr size_t SVK_SLOT_CONV32 = 96;         // svk_c3d2_conv32t (1 word)
constexpr size_t SVK_SLOT_CONV41 = 100;        // svk_c3d2_conv41 (1 word)
constexpr size_t SVK_SLOT_STAGE1 = 112;        // svk_c3d2_stage1 / svk_c3d2_stage1_c3 (1 word)
constexpr size_t SVK_SLOT_TOP1 = 120;          // svk_top1: the hit counter (1 u64)
constexpr size_t SVK_SLOT_HEAD = 128;          // svk_c3d2_head: the hit counters of ranks 1 .. 8 (8 u64)
static_assert(SVK_SLOT_STAGE2 + 8 <= SVK_SLOT_CONV31 && SVK_SLOT_STAGE1 + 4 <= SVK_SLOT_TOP1 && SVK_SLOT_TOP1 % 8 == 0 &&
                  SVK_SLOT_TOP1 + 8 <= SVK_SLOT_HEAD && SVK_SLOT_HEAD % 8 == 0 && SVK_SLOT_HEAD + 64 <= SVK_SCRATCH_BYTES,
              "the scratch slots overlap or do not fit the handle's scratch");

inline int svk_fail(svk_ctx* ctx, int code, const char* fmt, ...) {
  if (ctx) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(ctx->err, sizeof(ctx->err), fmt, ap);
    va_end(ap);
  }
  return code;
}

// Grow-only workspace.  Kernels using it are ordered on ctx->stream; growing frees the old block
// only after the stream has drained.
inline int svk_ensure_work(svk_ctx* ctx, size_t bytes) {
  if (ctx->work_bytes >= bytes) return SVK_OK;
  if (ctx->work) {
    if (hipStreamSynchronize(ctx->stream) != hipSuccess) return svk_fail(ctx, SVK_ERR_HIP, "stream sync before workspace growth failed");
    (void)hipFree(ctx->work);
    ctx->work = nullptr;
    ctx->work_bytes = 0;
  }
  const size_t want = (bytes + 4095) & ~(size_t)4095;
  if (hipMalloc(&ctx->work, want) != hipSuccess) return svk_fail(ctx, SVK_ERR_OOM, "workspace of %zu bytes", want);
  ctx->work_bytes = want;
  return SVK_OK;
}

#define SVK_HIP(ctx, call)                                                                      \
  do {                                                                                          \
    hipError_t e_ = (call);                                                                     \
    if (e_ != hipSuccess)                                                                       \
      return svk_fail((ctx), SVK_ERR_HIP, "%s failed: %s (%s:%d)", #call, hipGetErrorString(e_), \
                      __FILE__, __LINE__);                                                      \
  } while (0)

#define SVK_REQUIRE(ctx, cond, msg)                                                   \
  do {                                                                                \
    if (!(cond)) return svk_fail((ctx), SVK_ERR_BAD_ARG, "bad argument: %s", (msg));  \
  } while (0)

// p does not lie on a multiple of a bytes (a: a power of two); NULL is aligned to everything
inline bool misaligned(const void* p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) != 0; }

// Every launch is followed by this: catches bad grids / missing code objects at once.
#define SVK_LAUNCH_CHECK(ctx)                                                                  \
  do {                                                                                         \
    hipError_t e_ = hipGetLastError();                                                         \
    if (e_ != hipSuccess)                                                                      \
      return svk_fail((ctx), SVK_ERR_HIP, "kernel launch failed: %s (%s:%d)",                  \
                      hipGetErrorString(e_), __FILE__, __LINE__);                              \
  } while (0)

// The work-item counters of a persistent network kernel: `words` counters at byte `slot` of the handle's scratch, zeroed in
// stream order -- or nullptr (items at a fixed stride) while SVK_C3D2_STATIC_ITEMS is set, read at every call: the determinism
// tests set it at run time.
inline int svk_work_queue(svk_ctx* ctx, size_t slot, int words, unsigned** queue) {
  *queue = nullptr;
  if (getenv("SVK_C3D2_STATIC_ITEMS")) return SVK_OK;
  *queue = reinterpret_cast<unsigned*>(static_cast<char*>(ctx->scratch) + slot);
  SVK_HIP(ctx, hipMemsetAsync(*queue, 0, sizeof(unsigned) * words, ctx->stream));
  return SVK_OK;
}

// Launch width of a persistent network kernel: checks that `lds` bytes of dynamic LDS fit a CU beside the kernel's static LDS,
// raises the kernel's limit to them, and returns in *grid the `items` clamped to the workgroups resident at once -- one per CU
// when max_per_cu is 1, else what the occupancy calculator allows for `threads`-wide workgroups, at most max_per_cu.
template <class P>
int svk_persistent_grid(svk_ctx* ctx, const char* name, void (*kern)(P), size_t lds, int threads, int max_per_cu, int64_t items,
                        unsigned* grid) {
  if (lds + 64 > (size_t)ctx->lds_per_cu)
    return svk_fail(ctx, SVK_ERR_UNSUPPORTED, "%s needs %zu bytes of LDS per workgroup (device: %d)", name, lds, ctx->lds_per_cu);
  const void* f = reinterpret_cast<const void*>(kern);
  SVK_HIP(ctx, hipFuncSetAttribute(f, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  int per_cu = 1;
  if (max_per_cu > 1) {
    SVK_HIP(ctx, hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, f, threads, lds));
    per_cu = std::max(1, std::min(per_cu, max_per_cu));
  }
  *grid = (unsigned)std::min<int64_t>(items, (int64_t)per_cu * ctx->num_cu);
  return SVK_OK;
}

// out[row] = 1 / ||x[row]|| for the n rows of x, a zero norm as 1, on the handle's stream (scoring.hip's inv_norm_kernel: the
// pre-pass of the tiled cosine product and of the search, which runs it on both operands).  The caller checks the launch.
void svk_launch_inv_norm(svk_ctx* ctx, const float* d_x, int n, int dim, float* d_out);

// 64-lane wave sum; every lane gets the total.
__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
  return v;
}
__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
  return v;
}
__device__ __forceinline__ long long wave_sum(long long v) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
  return v;
}
