// Event frames (include/ren_amd.h "event frames"): recorded events -> per-window count images, and the per-window sums that
// compare the measured brightness change c_p n+ - c_n n- with a predicted one.
//
// Kernel A, event_frames_kernel: one event per lane per trip of a grid-stride loop.  An event costs 13 bytes of reads (one
// 32-bit word x | y << 16, an int64 timestamp, a polarity byte), all three streams coalesced; its window is the upper bound
// of its timestamp in the V + 1 edges (binary search; the edges are staged in LDS while V + 1 <= REN_EVENT_FRAMES_LDS_EDGES
// and read from global memory above that), and it adds 1 to one int32 counter with a no-return global atomic.  The stream is
// time-ordered, so the lanes of a wave search the same few edges (LDS broadcasts) but land on scattered pixels of one window's
// two planes.  Integer adds commute exactly: the counts do not depend on arrival order and repeated calls are bitwise equal.
// REN_EVENT_FRAMES_MERGE: before the atomic, the lanes of a wave that hold the same counter elect one lane that adds their
// number -- a loop over the wave's distinct counters (ballot / readlane), one atomic per distinct counter.  Same counts.
//
// Kernel B, two launches as ren_ssim_planes: event_compare_tile_kernel gives every workgroup TILE consecutive pixels of one
// window and forms the nine sums of the header in fp64 per thread, per wave (shuffles), per workgroup (LDS) in a fixed order;
// event_compare_window_kernel adds a window's tile partials in a fixed order.  No float atomics: bitwise repeatable.
// This file is compiled without FMA contraction, so m = c_p n+ - c_n n- and the products of the sums round term by term
// as a float64 restatement does.
#include "ren_common.h"

namespace {

constexpr int EF_THREADS = 256, EF_MAX_BLOCKS = 2048;
constexpr int CMP_THREADS = 256, CMP_WAVES = CMP_THREADS / REN_WAVE, CMP_PER_THREAD = 8, CMP_TILE = CMP_THREADS * CMP_PER_THREAD;
constexpr int CMP_SUMS = 9;

// index of the window that holds ts: (first i with edges[i] > ts) - 1, in [-1, n_edges - 1]
template <typename EdgePtr>
__device__ __forceinline__ int window_of(EdgePtr edges, int n_edges, int64_t ts) {
    int lo = 0, hi = n_edges;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (edges[mid] <= ts) lo = mid + 1;
        else hi = mid;
    }
    return lo - 1;
}

template <bool STAGED, bool MERGE>
__global__ void __launch_bounds__(EF_THREADS) event_frames_kernel(const uint32_t *__restrict__ position,
                                                                  const int64_t *__restrict__ timestamp,
                                                                  const uint8_t *__restrict__ polarity, int64_t N,
                                                                  const int64_t *__restrict__ edges, int V, int H, int W,
                                                                  int32_t *__restrict__ counts) {
    extern __shared__ int64_t s_edges[];                     // (V + 1) edges when STAGED (the only LDS of this kernel)
    const int n_edges = V + 1;
    if (STAGED) {
        for (int i = threadIdx.x; i < n_edges; i += EF_THREADS) s_edges[i] = edges[i];
        __syncthreads();
    }
    const int64_t plane = (int64_t)H * W, stride = (int64_t)gridDim.x * EF_THREADS;
    // the loop bound is the same for every lane of a workgroup, so the ballots of the merging form see whole waves
    for (int64_t base = (int64_t)blockIdx.x * EF_THREADS; base < N; base += stride) {
        const int64_t e = base + threadIdx.x;
        int64_t idx = -1;                                    // the counter this lane adds to, -1: none
        if (e < N) {
            const uint32_t xy = position[e];
            const int x = (int)(xy & 0xffffu), y = (int)(xy >> 16);
            const int64_t ts = timestamp[e];
            const int v = STAGED ? window_of(s_edges, n_edges, ts) : window_of(edges, n_edges, ts);
            if (v >= 0 && v < V && x < W && y < H)
                idx = ((int64_t)v * 2 + (polarity[e] ? 0 : 1)) * plane + (int64_t)y * W + x;
        }
        if (!MERGE) {
            if (idx >= 0) atomicAdd(counts + idx, 1);
        } else {
            const int lane = threadIdx.x & (REN_WAVE - 1);
            bool todo = idx >= 0;
            for (;;) {
                const unsigned long long live = __ballot(todo);
                if (!live) break;
                const int leader = __ffsll(live) - 1;
                const int64_t target = __shfl(idx, leader, REN_WAVE);
                const bool same = todo && idx == target;
                const unsigned long long group = __ballot(same);
                if (lane == leader) atomicAdd(counts + target, (int)__popcll(group));
                todo = todo && !same;
            }
        }
    }
}

__device__ __forceinline__ double wave_sum_f64(double v) {
    // butterfly over the 64 lanes; every lane ends with the same total, formed in the same order on every call
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, REN_WAVE);
    return v;
}

// the nine sums of one workgroup: wave butterflies, then the four waves in order; thread 0 writes them to out[0 .. 8]
__device__ __forceinline__ void block_sums(double (&s)[CMP_SUMS], double *__restrict__ out) {
    __shared__ double red[CMP_WAVES][CMP_SUMS];
    const int tid = threadIdx.x, lane = tid & (REN_WAVE - 1), wave = tid >> 6;
#pragma unroll
    for (int k = 0; k < CMP_SUMS; ++k) {
        s[k] = wave_sum_f64(s[k]);
        if (lane == 0) red[wave][k] = s[k];
    }
    __syncthreads();
    if (tid < CMP_SUMS) out[tid] = ((red[0][tid] + red[1][tid]) + red[2][tid]) + red[3][tid];
}

__global__ void __launch_bounds__(CMP_THREADS) event_compare_tile_kernel(const int32_t *__restrict__ counts,
                                                                         const float *__restrict__ pred,
                                                                         const uint8_t *__restrict__ valid, int64_t plane,
                                                                         int tiles_per_window, double c_p, double c_n,
                                                                         double c_max, double *__restrict__ partial) {
    const int64_t v = blockIdx.x / tiles_per_window;
    const int tile = blockIdx.x - (int)(v * tiles_per_window);
    const int32_t *pos = counts + v * 2 * plane, *neg = pos + plane;
    const float *P = pred + v * plane;
    const uint8_t *ok = valid + v * plane;
    double s[CMP_SUMS];
#pragma unroll
    for (int k = 0; k < CMP_SUMS; ++k) s[k] = 0.0;
#pragma unroll
    for (int j = 0; j < CMP_PER_THREAD; ++j) {
        const int64_t i = (int64_t)tile * CMP_TILE + j * CMP_THREADS + threadIdx.x;
        if (i < plane && ok[i]) {
            const int32_t np = pos[i], nn = neg[i];
            const double m = c_p * (double)np - c_n * (double)nn, p = (double)P[i], d = p - m;
            s[0] += 1.0;
            s[1] += m;
            s[2] += p;
            s[3] += m * m;
            s[4] += p * p;
            s[5] += m * p;
            s[6] += d * d;
            s[7] += fabs(d) <= c_max ? 1.0 : 0.0;
            s[8] += (np != 0 || nn != 0) ? 1.0 : 0.0;
        }
    }
    block_sums(s, partial + (int64_t)blockIdx.x * CMP_SUMS);
}

__global__ void __launch_bounds__(CMP_THREADS) event_compare_window_kernel(const double *__restrict__ partial,
                                                                           int tiles_per_window, double *__restrict__ out) {
    const double *src = partial + (int64_t)blockIdx.x * tiles_per_window * CMP_SUMS;
    double s[CMP_SUMS];
#pragma unroll
    for (int k = 0; k < CMP_SUMS; ++k) s[k] = 0.0;
    for (int i = threadIdx.x; i < tiles_per_window; i += CMP_THREADS)
#pragma unroll
        for (int k = 0; k < CMP_SUMS; ++k) s[k] += src[(int64_t)i * CMP_SUMS + k];
    block_sums(s, out + (int64_t)blockIdx.x * CMP_SUMS);
}

bool frame_shape_ok(int32_t V, int32_t H, int32_t W) { return V >= 1 && H >= 1 && W >= 1; }

int64_t compare_tiles(int32_t H, int32_t W) { return ((int64_t)H * W + CMP_TILE - 1) / CMP_TILE; }

template <bool MERGE>
void launch_event_frames(bool staged, int blocks, hipStream_t st, const uint32_t *position, const int64_t *timestamp,
                         const uint8_t *polarity, int64_t N, const int64_t *edges, int V, int H, int W, int32_t *counts) {
    auto staged_kernel = event_frames_kernel<true, MERGE>;
    auto global_kernel = event_frames_kernel<false, MERGE>;
    if (staged)
        hipLaunchKernelGGL(staged_kernel, dim3(blocks), dim3(EF_THREADS), (size_t)(V + 1) * sizeof(int64_t), st, position, timestamp,
                           polarity, N, edges, V, H, W, counts);
    else
        hipLaunchKernelGGL(global_kernel, dim3(blocks), dim3(EF_THREADS), 0, st, position, timestamp, polarity, N, edges, V, H, W,
                           counts);
}

}  // namespace

extern "C" int ren_event_frames(const uint32_t *position, const int64_t *timestamp, const uint8_t *polarity, int64_t N,
                                const int64_t *edges, int32_t V, int32_t H, int32_t W, int32_t flags, int32_t *counts,
                                void *stream) {
    if (!edges || !counts || N < 0) return REN_ERR_BAD_ARG;
    if (!frame_shape_ok(V, H, W)) return REN_ERR_BAD_ARG;
    if (N > 0 && (!position || !timestamp || !polarity)) return REN_ERR_BAD_ARG;
    if (flags & ~REN_EVENT_FRAMES_MERGE) return REN_ERR_BAD_ARG;
    if (H > 65536 || W > 65536 || V == INT32_MAX) return REN_ERR_UNSUPPORTED;        // coordinates are 16 bits; V + 1 is an int
    if (N == 0) return REN_OK;
    const bool staged = (int64_t)V + 1 <= REN_EVENT_FRAMES_LDS_EDGES;
    const int64_t want = (N + EF_THREADS - 1) / EF_THREADS;
    const int blocks = (int)(want < EF_MAX_BLOCKS ? want : EF_MAX_BLOCKS);
    if (flags & REN_EVENT_FRAMES_MERGE)
        launch_event_frames<true>(staged, blocks, (hipStream_t)stream, position, timestamp, polarity, N, edges, V, H, W, counts);
    else
        launch_event_frames<false>(staged, blocks, (hipStream_t)stream, position, timestamp, polarity, N, edges, V, H, W, counts);
    REN_CHECK_LAUNCH();
}

extern "C" int64_t ren_event_frame_compare_scratch_doubles(int32_t V, int32_t H, int32_t W) {
    if (!frame_shape_ok(V, H, W)) return 0;
    return (int64_t)V * compare_tiles(H, W) * CMP_SUMS;
}

extern "C" int ren_event_frame_compare(const int32_t *counts, const float *pred, const uint8_t *valid, int32_t V, int32_t H,
                                       int32_t W, double c_p, double c_n, double *out, double *scratch, void *stream) {
    if (!counts || !pred || !valid || !out || !scratch) return REN_ERR_BAD_ARG;
    if (!frame_shape_ok(V, H, W)) return REN_ERR_BAD_ARG;
    if (!(std::isfinite(c_p) && std::isfinite(c_n))) return REN_ERR_BAD_ARG;
    const int64_t tiles = compare_tiles(H, W);
    if ((int64_t)V * tiles > INT32_MAX) return REN_ERR_UNSUPPORTED;
    const double c_max = c_p > c_n ? c_p : c_n;
    hipLaunchKernelGGL(event_compare_tile_kernel, dim3((unsigned)(V * tiles)), dim3(CMP_THREADS), 0, (hipStream_t)stream, counts,
                       pred, valid, (int64_t)H * W, (int)tiles, c_p, c_n, c_max, scratch);
    if (hipGetLastError() != hipSuccess) return REN_ERR_LAUNCH;
    hipLaunchKernelGGL(event_compare_window_kernel, dim3((unsigned)V), dim3(CMP_THREADS), 0, (hipStream_t)stream, scratch,
                       (int)tiles, out);
    REN_CHECK_LAUNCH();
}
