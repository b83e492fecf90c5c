// Event filter (include/ren_amd.h "event filter"): which events of a raw stream are scene signal -- not at a hot pixel, and
// SUPPORTED by another event at one of the eight neighbouring pixels (nine with include_self) no more than dt earlier -- on the
// structure the table build leaves behind: the int32 pixel keys in stable by-pixel order, `order` back to stream order, and the
// timestamps gathered into that order (ts_sorted), whose per-pixel segments [seg[p], seg[p + 1]) are time-ordered because the
// stream is.
//
// One kernel, event_support_kernel: one sorted slot per lane per trip of a grid-stride loop.  Slot i reads its key, its stream
// index and its own time (20 B, coalesced) and the hot flag of its pixel (1 B; lanes of a wave share a few pixels).  For each
// in-sensor neighbour pixel it reads the hot flag (1 B) and the two segment bounds (8 B), then binary-searches the segment of
// ts_sorted for the last t' <= t: an upper bound, ceil(log2(length + 1)) DEPENDENT 8-B loads, and t - t' <= dt decides.  It stops
// at the first neighbour that passes and scatters one byte to keep[order[i]] (every stream index exactly once: order is a
// permutation).  Per event at most 21 B + 8 (9) x (9 B + 8 B x ceil(log2(length + 1))) read and 1 B written; with c events per
// pixel that is up to 8 ceil(log2(c + 1)) dependent loads, fewer where an early neighbour passes.
// Locality (reasoning, not a measurement): adjacent lanes hold adjacent slots, i.e. events adjacent in time at the SAME pixel,
// so their searches run over the same eight segments, take the same first probes and end in adjacent slots of them; the lines
// one lane pulls in are the lines its neighbours need.
// Own pixel (include_self): the upper bound over the pixel's own segment lands on slot i or, when later events there carry the
// same timestamp, past it (t' = t: they support i); when it lands on i the candidate is slot i - 1 of the same segment.
// All time differences are signed 64-bit.  Segment bounds read from memory are clamped to [0, N] before anything is read
// through them.  No LDS, no atomics, no workgroup waits on another.
#include "ren_common.h"

namespace {

constexpr int EF_THREADS = REN_EVENT_FILTER_THREADS, EF_MAX_BLOCKS = REN_EVENT_FILTER_MAX_BLOCKS;

__global__ void __launch_bounds__(EF_THREADS) event_support_kernel(const int32_t *__restrict__ pix_sorted,
                                                                   const int64_t *__restrict__ order,
                                                                   const int64_t *__restrict__ ts_sorted,
                                                                   const int32_t *__restrict__ seg,
                                                                   const uint8_t *__restrict__ hot, int64_t N, int H, int W,
                                                                   int64_t dt, int include_self, uint8_t *__restrict__ keep) {
    const int64_t stride = (int64_t)gridDim.x * EF_THREADS;
    const int64_t pixels = (int64_t)H * W;
    for (int64_t i = (int64_t)blockIdx.x * EF_THREADS + threadIdx.x; i < N; i += stride) {
        const int64_t j = order[i];
        if ((uint64_t)j >= (uint64_t)N) continue;            // not a stream index: nothing is read or written for it
        const int64_t p = pix_sorted[i];
        bool ok = (uint64_t)p < (uint64_t)pixels && !(hot && hot[p]);       // a key outside the sensor is not kept
        if (ok && dt >= 0) {                                  // dt < 0: no support test
            ok = false;
            const int64_t t = ts_sorted[i];
            const int y = (int)(p / W), x = (int)(p - (int64_t)y * W);
            for (int k = 0; k < 9 && !ok; ++k) {
                const int yy = y + k / 3 - 1, xx = x + k % 3 - 1;
                if (yy < 0 || yy >= H || xx < 0 || xx >= W) continue;
                const int64_t q = (int64_t)yy * W + xx;
                if (q == p ? !include_self : (hot && hot[q])) continue;
                int64_t lo = seg[q], hi = seg[q + 1];
                lo = lo < 0 ? 0 : lo;
                hi = hi > N ? N : hi;
                const int64_t first = lo;
                while (lo < hi) {                             // upper bound: the first slot of the segment with a time > t
                    const int64_t mid = lo + ((hi - lo) >> 1);
                    if (ts_sorted[mid] <= t) lo = mid + 1; else hi = mid;
                }
                int64_t c = lo - 1;                           // the last slot with a time <= t
                if (q == p && c == i) c = i - 1;              // the event itself: the one before it at this pixel
                if (c < first) continue;
                const int64_t d = t - ts_sorted[c];
                ok = d >= 0 && d <= dt;
            }
        }
        keep[j] = ok ? 1 : 0;
    }
}

bool misaligned(const void *p, uintptr_t bytes) { return ((uintptr_t)p & (bytes - 1)) != 0; }

}  // namespace

extern "C" int ren_event_support(const int32_t *pix_sorted, const int64_t *order, const int64_t *ts_sorted, const int32_t *seg,
                                 const uint8_t *hot, int64_t N, int32_t H, int32_t W, int64_t dt, int32_t include_self,
                                 uint8_t *keep, void *stream) {
    if (N < 0 || H < 1 || W < 1 || (include_self != 0 && include_self != 1)) return REN_ERR_BAD_ARG;
    if (N > 0 && (!pix_sorted || !order || !ts_sorted || !seg || !keep)) return REN_ERR_BAD_ARG;
    if (misaligned(pix_sorted, 4) || misaligned(order, 8) || misaligned(ts_sorted, 8) || misaligned(seg, 4)) return REN_ERR_BAD_ARG;
    if (N > INT32_MAX || (int64_t)H * W > INT32_MAX) return REN_ERR_UNSUPPORTED;
    if (N == 0) return REN_OK;
    const int64_t want = (N + EF_THREADS - 1) / EF_THREADS;
    const int blocks = (int)(want < EF_MAX_BLOCKS ? want : EF_MAX_BLOCKS);
    hipLaunchKernelGGL(event_support_kernel, dim3(blocks), dim3(EF_THREADS), 0, (hipStream_t)stream, pix_sorted, order, ts_sorted,
                       seg, hot, N, (int)H, (int)W, dt, (int)include_self, keep);
    REN_CHECK_LAUNCH();
}
