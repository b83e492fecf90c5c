// Event table (include/ren_amd.h "event table"): raw_events.npz -> the per-pixel (start_ts, end_ts, polarity) intervals the
// training draws its batches from, with Bayer channel and undistorted position, and tau_max = the minimum interval -- after
// ONE stable sort of the int32 pixel keys (the caller's: torch.sort) and a prefix sum of the keep flags.
//
// Kernel 1, event_intervals_kernel: one sorted slot per lane per trip of a grid-stride loop.  Slot i reads its key and its
// left neighbour's (coalesced; the neighbour's word is the previous lane's), its stream index j = order[i] and order[i - 1]
// (the same), and gathers ts[j] and ts[order[i - 1]] (the second is the previous slot's first: a cache hit).  It scatters the
// keep flag to valid[j] (every j exactly once: order is a permutation) and, for a kept event, the predecessor's time to
// start_ts[j].  Per event: 12 B of coalesced reads, one 8-B gather, a 1-B scatter, an 8-B scatter per kept event.  The
// comparison is with the IMMEDIATE predecessor in the by-pixel order, kept or not, as data.queue_raw_events does.
// The minimum of the kept differences (signed int64) is reduced per lane over the trips, per wave (shuffles), per workgroup
// (LDS), then ONE 64-bit vector atomicMin per workgroup into the caller's word; a minimum does not depend on the order of
// its operands, so the word is bitwise repeatable.  No workgroup waits on another.
//
// Kernel 2, event_table_write_kernel: one stream event per lane per trip.  A kept event e writes row offsets[e] of the
// table: position from the (H * W, 2) float32 lookup table at its pixel or a plain cast, start_ts, end_ts, num_pos = p,
// num_neg = 1 - p, and the Bayer channel of (x & 1) + 2 (y & 1).  Rows are written in stream order, so with most events kept
// the five (six) output streams are nearly contiguous per wave.  Reads per event: 1 (flag) + 4 (offset) + 2 * sizeof(stored
// coordinate), and per kept event 8 + 8 + 1 + an 8-B table gather; writes per kept event 40 (41) B.
#include "ren_common.h"

namespace {

constexpr int ET_THREADS = REN_EVENT_TABLE_THREADS, ET_WAVES = ET_THREADS / REN_WAVE, ET_MAX_BLOCKS = 2048;
constexpr long long ET_NONE = INT64_MAX;

__global__ void __launch_bounds__(ET_THREADS) event_intervals_kernel(const int32_t *__restrict__ pix_sorted,
                                                                     const int64_t *__restrict__ order,
                                                                     const int64_t *__restrict__ ts, int64_t N,
                                                                     uint8_t *__restrict__ valid, int64_t *__restrict__ start_ts,
                                                                     long long *__restrict__ min_diff) {
    __shared__ long long red[ET_WAVES];
    const int64_t stride = (int64_t)gridDim.x * ET_THREADS;
    long long best = ET_NONE;
    for (int64_t i = (int64_t)blockIdx.x * ET_THREADS + threadIdx.x; i < N; i += stride) {
        const int64_t j = order[i];
        if ((uint64_t)j >= (uint64_t)N) continue;            // not a stream index: nothing is read or written for it
        bool keep = false;
        if (i > 0 && pix_sorted[i] == pix_sorted[i - 1]) {
            const int64_t jp = order[i - 1];
            if ((uint64_t)jp < (uint64_t)N) {
                const int64_t tp = ts[jp];
                const long long d = (long long)(ts[j] - tp);
                if (d != 0) {
                    keep = true;
                    start_ts[j] = tp;
                    best = d < best ? d : best;
                }
            }
        }
        valid[j] = keep ? 1 : 0;
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const long long o = __shfl_xor(best, off, REN_WAVE);
        best = o < best ? o : best;
    }
    const int lane = threadIdx.x & (REN_WAVE - 1), wave = threadIdx.x >> 6;
    if (lane == 0) red[wave] = best;
    __syncthreads();
    if (threadIdx.x == 0) {
        long long m = red[0];
#pragma unroll
        for (int w = 1; w < ET_WAVES; ++w) m = red[w] < m ? red[w] : m;
        if (m != ET_NONE) atomicMin(min_diff, m);
    }
}

template <typename PosT> struct pos_pair;
template <> struct pos_pair<uint16_t> { using type = ushort2; };
template <> struct pos_pair<int32_t> { using type = int2; };
template <> struct pos_pair<int64_t> { using type = longlong2; };

template <typename PosT>
__global__ void __launch_bounds__(ET_THREADS) event_table_write_kernel(
    const uint8_t *__restrict__ valid, const int32_t *__restrict__ offsets, const typename pos_pair<PosT>::type *__restrict__ position,
    const int64_t *__restrict__ ts, const int64_t *__restrict__ start_ts, const uint8_t *__restrict__ polarity, int64_t N, int64_t M,
    const float2 *__restrict__ lut, int H, int W, uint32_t channels, float2 *__restrict__ out_position,
    int64_t *__restrict__ out_start, int64_t *__restrict__ out_end, int64_t *__restrict__ out_num_pos,
    int64_t *__restrict__ out_num_neg, uint8_t *__restrict__ out_channel) {
    const int64_t stride = (int64_t)gridDim.x * ET_THREADS;
    for (int64_t e = (int64_t)blockIdx.x * ET_THREADS + threadIdx.x; e < N; e += stride) {
        if (!valid[e]) continue;
        const int64_t m = offsets[e];
        if ((uint64_t)m >= (uint64_t)M) continue;            // a row the caller did not allocate is not written
        const auto xy = position[e];
        const int64_t x = (int64_t)xy.x, y = (int64_t)xy.y;
        float2 p = make_float2((float)xy.x, (float)xy.y);
        // the caller has checked 0 <= x < W, 0 <= y < H (data.build_event_table); the gather never leaves the table regardless
        if (lut && (uint64_t)x < (uint64_t)W && (uint64_t)y < (uint64_t)H) p = lut[y * W + x];
        const int64_t pol = (int64_t)polarity[e];
        out_position[m] = p;
        out_start[m] = start_ts[e];
        out_end[m] = ts[e];
        out_num_pos[m] = pol;
        out_num_neg[m] = 1 - pol;
        if (out_channel) out_channel[m] = (uint8_t)(channels >> (8 * (int)((x & 1) + 2 * (y & 1))));     // TL, TR, BL, BR
    }
}

int table_blocks(int64_t n) {
    const int64_t want = (n + ET_THREADS - 1) / ET_THREADS;
    return (int)(want < ET_MAX_BLOCKS ? want : ET_MAX_BLOCKS);
}

bool misaligned(const void *p, uintptr_t bytes) { return ((uintptr_t)p & (bytes - 1)) != 0; }

template <typename PosT>
void launch_table_write(hipStream_t st, const uint8_t *valid, const int32_t *offsets, const void *position, const int64_t *ts,
                        const int64_t *start_ts, const uint8_t *polarity, int64_t N, int64_t M, const float *lut, int H, int W,
                        uint32_t channels, float *out_position, int64_t *out_start, int64_t *out_end, int64_t *out_num_pos,
                        int64_t *out_num_neg, uint8_t *out_channel) {
    hipLaunchKernelGGL(event_table_write_kernel<PosT>, dim3(table_blocks(N)), dim3(ET_THREADS), 0, st, valid, offsets,
                       (const typename pos_pair<PosT>::type *)position, ts, start_ts, polarity, N, M, (const float2 *)lut, H, W,
                       channels, (float2 *)out_position, out_start, out_end, out_num_pos, out_num_neg, out_channel);
}

}  // namespace

extern "C" int ren_event_intervals(const int32_t *pix_sorted, const int64_t *order, const int64_t *timestamp, int64_t N,
                                   uint8_t *valid, int64_t *start_ts, int64_t *min_diff, void *stream) {
    if (N < 0 || !min_diff || misaligned(min_diff, 8)) return REN_ERR_BAD_ARG;
    if (N > 0 && (!pix_sorted || !order || !timestamp || !valid || !start_ts)) return REN_ERR_BAD_ARG;
    if (misaligned(pix_sorted, 4) || misaligned(order, 8) || misaligned(timestamp, 8) || misaligned(start_ts, 8))
        return REN_ERR_BAD_ARG;
    if (N > INT32_MAX) return REN_ERR_UNSUPPORTED;
    if (N == 0) return REN_OK;
    hipLaunchKernelGGL(event_intervals_kernel, dim3(table_blocks(N)), dim3(ET_THREADS), 0, (hipStream_t)stream, pix_sorted, order,
                       timestamp, N, valid, start_ts, (long long *)min_diff);
    REN_CHECK_LAUNCH();
}

extern "C" int ren_event_table_write(const uint8_t *valid, const int32_t *offsets, const void *position, int32_t position_bytes,
                                     const int64_t *timestamp, const int64_t *start_ts, const uint8_t *polarity, int64_t N,
                                     int64_t M, const float *lut, int32_t H, int32_t W, const uint8_t *bayer_channels,
                                     float *out_position, int64_t *out_start_ts, int64_t *out_end_ts, int64_t *out_num_pos,
                                     int64_t *out_num_neg, uint8_t *out_channel_idx, void *stream) {
    if (N < 0 || M < 0 || M > N || H < 1 || W < 1) return REN_ERR_BAD_ARG;
    if (position_bytes != 2 && position_bytes != 4 && position_bytes != 8) return REN_ERR_BAD_ARG;
    if ((bayer_channels != nullptr) != (out_channel_idx != nullptr)) return REN_ERR_BAD_ARG;
    if (N > 0 && (!valid || !offsets || !position || !timestamp || !start_ts || !polarity)) return REN_ERR_BAD_ARG;
    if (M > 0 && (!out_position || !out_start_ts || !out_end_ts || !out_num_pos || !out_num_neg)) return REN_ERR_BAD_ARG;
    if (misaligned(offsets, 4) || misaligned(position, 2 * (uintptr_t)position_bytes) || misaligned(timestamp, 8) ||
        misaligned(start_ts, 8) || misaligned(lut, 8) || misaligned(out_position, 8) || misaligned(out_start_ts, 8) ||
        misaligned(out_end_ts, 8) || misaligned(out_num_pos, 8) || misaligned(out_num_neg, 8))
        return REN_ERR_BAD_ARG;
    if (N > INT32_MAX || (int64_t)H * W > INT32_MAX) return REN_ERR_UNSUPPORTED;
    if (N == 0 || M == 0) return REN_OK;
    uint32_t channels = 0;
    if (bayer_channels)
        for (int k = 0; k < 4; ++k) channels |= (uint32_t)bayer_channels[k] << (8 * k);
    hipStream_t st = (hipStream_t)stream;
    if (position_bytes == 2)
        launch_table_write<uint16_t>(st, valid, offsets, position, timestamp, start_ts, polarity, N, M, lut, H, W, channels,
                                     out_position, out_start_ts, out_end_ts, out_num_pos, out_num_neg, out_channel_idx);
    else if (position_bytes == 4)
        launch_table_write<int32_t>(st, valid, offsets, position, timestamp, start_ts, polarity, N, M, lut, H, W, channels,
                                    out_position, out_start_ts, out_end_ts, out_num_pos, out_num_neg, out_channel_idx);
    else
        launch_table_write<int64_t>(st, valid, offsets, position, timestamp, start_ts, polarity, N, M, lut, H, W, channels,
                                    out_position, out_start_ts, out_end_ts, out_num_pos, out_num_neg, out_channel_idx);
    REN_CHECK_LAUNCH();
}
