// The static voicepack's table on the device (train/voicepack.py:116-136, make_static): every utterance's style row
// [D = 192] is filed under bucket text_length - 1 of `rows` (512) buckets, and row i of the pack is the mean over the
// rows of the buckets in a window around i.  The reference keeps Python lists of device tensors and averages them in
// fp32 (torch.stack(...).mean(0)) once per row of the pack; here the table is float64 sums + int64 counts that stay on
// the device for the whole pass over the dataset, so the loop never waits for the host: only `counts` (4 KB) goes back,
// once, for the host to resolve the windows (voicepack.resolve_windows: the widening rule and its negative-slice quirk
// are host arithmetic on 512 integers).
//
// Determinism: column d of the table belongs to ONE thread per launch, which walks the batch in row order -- the rows of
// a bucket are added in the order they arrive, there is no float atomic, and two passes over the same batches give the
// same bits.  Launches on one stream are ordered, so the order across batches is the order of the calls.
#include "sty_common.h"

namespace sty {

constexpr int PACK_SEG = 8;  // bucket b is handled by blockIdx.y == b % PACK_SEG (a batch of one length bin hits few buckets)

// grid (ceil(D / 64), PACK_SEG), 64 threads: thread = one column d of the buckets of its segment
__global__ __launch_bounds__(64) void pack_accumulate_kernel(int n, int D, int rows, const float* __restrict__ styles,
                                                             const int64_t* __restrict__ text_lengths,
                                                             double* __restrict__ sums, int64_t* __restrict__ counts) {
  const int d = blockIdx.x * 64 + threadIdx.x;
  const int seg = blockIdx.y;
  if (d >= D) return;
  for (int i = 0; i < n; ++i) {
    const int64_t len = text_lengths[i];
    if (len < 1 || len > rows) continue;  // (the caller refuses such a batch on the host; never an out-of-bounds write)
    const int b = (int)len - 1;
    if (b % PACK_SEG != seg) continue;
    sums[(size_t)b * D + d] += (double)styles[(size_t)i * D + d];
    if (d == 0) counts[b] += 1;
  }
}

// one thread per (row i, column d): the window's buckets in ascending order, one division, one rounding to fp32
__global__ __launch_bounds__(256) void pack_finalize_kernel(int rows, int D, const double* __restrict__ sums,
                                                            const int64_t* __restrict__ counts,
                                                            const int32_t* __restrict__ lo, const int32_t* __restrict__ hi,
                                                            float* __restrict__ pack) {
  const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= (size_t)rows * D) return;
  const int i = (int)(idx / D), d = (int)(idx % D);
  int b0 = lo[i], b1 = hi[i];
  if (b0 < 0) b0 = 0;
  if (b1 > rows) b1 = rows;
  double s = 0.0;
  int64_t c = 0;
  for (int b = b0; b < b1; ++b) {
    const int64_t cb = counts[b];
    if (cb == 0) continue;  // an empty bucket holds +0.0: skipping it changes nothing and saves the load
    s += sums[(size_t)b * D + d];
    c += cb;
  }
  pack[idx] = (float)(s / (double)c);  // an empty window is 0 / 0 = NaN: the host resolves windows that hold rows
}

}  // namespace sty

extern "C" int sty_pack_accumulate(int n, int D, int rows, const float* styles, const int64_t* text_lengths, double* sums,
                                   int64_t* counts, void* stream) {
  using namespace sty;
  if (n < 0 || D < 1 || rows < 1 || (n > 0 && (!styles || !text_lengths)) || !sums || !counts) {
    set_error("sty_pack_accumulate: null buffer or n < 0 / D < 1 / rows < 1");
    return STY_EINVAL;
  }
  if (n == 0) return STY_OK;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  ProfScope prof("pack_accumulate_kernel", (double)n * D, (double)n * D * (4.0 + 16.0), st);
  hipLaunchKernelGGL(pack_accumulate_kernel, dim3((unsigned)cdiv(D, 64), PACK_SEG), dim3(64), 0, st, n, D, rows, styles,
                     text_lengths, sums, counts);
  STY_LAUNCH_CHECK();
  return STY_OK;
}

extern "C" int sty_pack_finalize(int rows, int D, const double* sums, const int64_t* counts, const int32_t* lo,
                                 const int32_t* hi, float* pack, void* stream) {
  using namespace sty;
  if (D < 1 || rows < 1 || !sums || !counts || !lo || !hi || !pack) {
    set_error("sty_pack_finalize: null buffer or D < 1 / rows < 1");
    return STY_EINVAL;
  }
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const size_t total = (size_t)rows * D;
  ProfScope prof("pack_finalize_kernel", (double)total * rows, (double)total * 4.0 + (double)total * 8.0, st);
  hipLaunchKernelGGL(pack_finalize_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, rows, D, sums, counts,
                     lo, hi, pack);
  STY_LAUNCH_CHECK();
  return STY_OK;
}
