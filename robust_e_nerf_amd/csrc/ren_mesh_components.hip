// Connected components of a density lattice (include/ren_amd.h "mesh components"): the solids of the level-set mesh -- and,
// with outside != 0, its voids -- labelled by their smallest lattice index, with their sizes and whether they touch the
// lattice's faces.  mesh.clean drops floaters and fills cavities with it before the unchanged extraction of ren_mesh.hip.
//
// Two points of the selected set S are joined when a marching-tetrahedra edge joins them: the seven forward directions of
// ren_mesh.hip and their opposites.  Union-find over the lattice with `label` as the parent array, three launches whatever
// the data, the kernel boundary the only synchronisation between them; no loop anywhere waits for another wave.
//
// Launch 1, init: label[p] = p for p in S, else -1; size[p] = 0, border[p] = 0.
// Launch 2, union: one point per lane.  The lane classifies itself and its seven forward neighbours from sigma (as
//   mesh_classify_kernel does, every neighbour range-checked) and unites itself with the forward neighbours in S.  A
//   diagonal whose far end is already reached over two edges that other lanes unite is left out: (1,1,0) when p + (1,0,0) or
//   p + (0,1,0) is in S (that point is joined to p by this lane and to p + (1,1,0) by its own lane), likewise (1,0,1) and
//   (0,1,1), and (1,1,1) when any of the six other neighbours is in S.  The components are those of all seven directions.
//   unite(a, b): both walk to a root; equal roots: done; otherwise the LARGER root is linked to the smaller by a
//   compare-and-swap that expects the larger root to be its own parent still; a failed swap returns the parent somebody else
//   gave it and the walk goes on from there.  A walk of two or more steps leaves the root it found in its starting point
//   (atomic min).  Every value ever stored in label[x] is <= x and an index of x's component, so (1) parents strictly descend:
//   no cycle, every walk ends after at most x steps, every failed swap moves to a strictly smaller index; (2) a link is made
//   only by a successful swap, which the memory side executes on the current value: the linked index was a root at that
//   instant; (3) a STALE parent -- an older value of label[x] from a cache that another XCD's store never refreshed -- is
//   still an index of the component that is <= x: the walk stops early or takes a longer way, and where it ends on an index
//   that is a root no more, the swap there fails and hands over the current parent.  Every read and write of label in this
//   launch is a relaxed atomic of agent scope.
// Launch 3, flatten: label[p] = root of p; the roots' sizes by integer atomic adds, one per distinct root of a wave; border[root]
//   = 1 by a plain store from every point on a face of the lattice (all writers store the same byte).  Walks here cross
//   labels that other lanes are replacing by their roots: either value is an index of the component that is <= x.
// The outputs are functions of (sigma, level, outside): they repeat bit for bit whatever order the atomics land in.
//
// ren_mesh_component_apply: one point per lane, out[p] = value where drop[label[p]] != 0, else the 32 bits of sigma[p].
#include "ren_common.h"
#include <string.h>

namespace {

constexpr int MC_THREADS = REN_MESH_THREADS;
constexpr uint32_t MC_CODE_OF_DIR = 0x7653421u;                                // corner code dx | dy << 1 | dz << 2 of direction e (nibble e)

#define MC_RELAXED __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT

__device__ __forceinline__ bool mc_selected(float s, float level, int outside) { return (s >= level) != (outside != 0); }

__device__ __forceinline__ void mc_coords(uint32_t p, int ny, int nz, int &i, int &j, int &k) {
    const uint32_t row = p / (uint32_t)nz;
    k = (int)(p - row * (uint32_t)nz);
    i = (int)(row / (uint32_t)ny);
    j = (int)(row - (uint32_t)i * (uint32_t)ny);
}

// the root above x: parents strictly descend (label[y] <= y), so the loop ends; a value that is no index cannot come from
// these kernels and ends the walk without being followed
__device__ __forceinline__ int32_t mc_find(int32_t *label, uint32_t n, int32_t x, int &steps) {
    steps = 0;
    for (;;) {
        const int32_t up = __hip_atomic_load(label + x, MC_RELAXED);
        if (up >= x || (uint32_t)up >= n) return x;
        x = up;
        ++steps;
    }
}

__device__ __forceinline__ void mc_unite(int32_t *label, uint32_t n, int32_t a, int32_t b) {
    const int32_t a0 = a, b0 = b;
    int sa, sb;
    a = mc_find(label, n, a, sa);
    b = mc_find(label, n, b, sb);
    while (a != b) {
        if (a < b) {
            const int32_t t = a;
            a = b;
            b = t;
        }
        int32_t seen = a;                                                       // link the larger root a under the smaller b
        if (__hip_atomic_compare_exchange_strong(label + a, &seen, b, __ATOMIC_RELAXED, MC_RELAXED)) break;
        if (seen >= a || (uint32_t)seen >= n) break;                            // not a value of these kernels: leave, never spin
        int s;
        a = mc_find(label, n, seen, s);                                         // a has a parent now: strictly below a
        sa = sb = 2;                                                            // both ends are at least two steps from the root
    }
    const int32_t root = a < b ? a : b;
    if (sa > 1) __hip_atomic_fetch_min(label + a0, root, MC_RELAXED);
    if (sb > 1) __hip_atomic_fetch_min(label + b0, root, MC_RELAXED);
}

__global__ void __launch_bounds__(MC_THREADS) mesh_components_init_kernel(const float *__restrict__ sigma, uint32_t n, float level,
                                                                          int outside, int32_t *__restrict__ label,
                                                                          int32_t *__restrict__ size, uint8_t *__restrict__ border) {
    const uint32_t p = blockIdx.x * (uint32_t)MC_THREADS + threadIdx.x;
    if (p >= n) return;
    label[p] = mc_selected(sigma[p], level, outside) ? (int32_t)p : -1;
    size[p] = 0;
    border[p] = 0;
}

__global__ void __launch_bounds__(MC_THREADS) mesh_components_union_kernel(const float *__restrict__ sigma, int nx, int ny, int nz,
                                                                           float level, int outside, int32_t *label) {
    const uint32_t n = (uint32_t)nx * (uint32_t)ny * (uint32_t)nz;             // <= 2^30 (checked by the host)
    const uint32_t p = blockIdx.x * (uint32_t)MC_THREADS + threadIdx.x;
    if (p >= n) return;
    if (!mc_selected(sigma[p], level, outside)) return;
    int i, j, k;
    mc_coords(p, ny, nz, i, j, k);
    const bool hx = i + 1 < nx, hy = j + 1 < ny, hz = k + 1 < nz;
    const int32_t sx = ny * nz, sy = nz;                                        // p + sx + sy + 1 < n <= 2^30 wherever it is formed
    uint32_t in8 = 0;                                                           // bit c: the neighbour with corner code c is in S
#pragma unroll
    for (int e = 0; e < 7; ++e) {
        const int c = (int)(MC_CODE_OF_DIR >> (4 * e) & 7u);
        if ((!(c & 1) || hx) && (!(c & 2) || hy) && (!(c & 4) || hz)) {
            const float s = sigma[(int32_t)p + ((c & 1) ? sx : 0) + ((c & 2) ? sy : 0) + ((c & 4) ? 1 : 0)];
            in8 |= (mc_selected(s, level, outside) ? 1u : 0u) << c;
        }
    }
    // the diagonals that two edges of other unions already span
    uint32_t todo = in8 & 0x16u;                                                // codes 1, 2, 4: the axes, always
    if ((in8 & 0x08u) && !(in8 & 0x06u)) todo |= 0x08u;                         // code 3 = x + y unless x or y is in S
    if ((in8 & 0x20u) && !(in8 & 0x12u)) todo |= 0x20u;                         // code 5 = x + z
    if ((in8 & 0x40u) && !(in8 & 0x14u)) todo |= 0x40u;                         // code 6 = y + z
    if ((in8 & 0x80u) && !(in8 & 0x7Eu)) todo |= 0x80u;                         // code 7 = x + y + z unless any other is in S
#pragma unroll
    for (int c = 1; c < 8; ++c)
        if (todo >> c & 1u)
            mc_unite(label, n, (int32_t)p, (int32_t)p + ((c & 1) ? sx : 0) + ((c & 2) ? sy : 0) + ((c & 4) ? 1 : 0));
}

__global__ void __launch_bounds__(MC_THREADS) mesh_components_flatten_kernel(int nx, int ny, int nz, int32_t *label, int32_t *size,
                                                                             uint8_t *border) {
    const uint32_t n = (uint32_t)nx * (uint32_t)ny * (uint32_t)nz;
    const uint32_t p = blockIdx.x * (uint32_t)MC_THREADS + threadIdx.x;
    int32_t root = -1;
    if (p < n && __hip_atomic_load(label + p, MC_RELAXED) >= 0) {
        int steps;
        root = mc_find(label, n, (int32_t)p, steps);
        if (steps > 0) __hip_atomic_store(label + p, root, MC_RELAXED);
        int i, j, k;
        mc_coords(p, ny, nz, i, j, k);
        if (i == 0 || j == 0 || k == 0 || i == nx - 1 || j == ny - 1 || k == nz - 1) border[root] = 1;
    }
    // one add per distinct root of the wave: at most 64 rounds, each of which retires the lanes of one root
    unsigned long long left = __ballot(root >= 0);
    const int lane = (int)(threadIdx.x & (REN_WAVE - 1));
    while (left) {
        const int lead = __ffsll(left) - 1;
        const int32_t r = __shfl(root, lead, REN_WAVE);
        const unsigned long long same = __ballot(root == r);
        if (lane == lead) atomicAdd(size + r, (int32_t)__popcll(same));
        left &= ~same;
    }
}

__global__ void __launch_bounds__(MC_THREADS) mesh_component_apply_kernel(const uint32_t *sigma, const int32_t *__restrict__ label,
                                                                          const uint8_t *__restrict__ drop, int64_t n, uint32_t value,
                                                                          uint32_t *out) {
    const int64_t p = (int64_t)blockIdx.x * MC_THREADS + threadIdx.x;
    if (p >= n) return;
    const int32_t l = label[p];
    const bool hit = l >= 0 && (int64_t)l < n && drop[l] != 0;                  // a label that is no index drops nothing
    out[p] = hit ? value : sigma[p];
}

bool mc_misaligned(const void *p, uintptr_t bytes) { return ((uintptr_t)p & (bytes - 1)) != 0; }

}  // namespace

extern "C" int ren_mesh_components(const float *sigma, int32_t nx, int32_t ny, int32_t nz, float level, int32_t outside,
                                   int32_t *label, int32_t *size, uint8_t *border, void *stream) {
    if (nx < 2 || ny < 2 || nz < 2 || (int64_t)nx * ny * nz > REN_MESH_MAX_POINTS || level != level) return REN_ERR_BAD_ARG;
    if (outside != 0 && outside != 1) return REN_ERR_BAD_ARG;
    if (!sigma || !label || !size || !border) return REN_ERR_BAD_ARG;
    if (mc_misaligned(sigma, 4) || mc_misaligned(label, 4) || mc_misaligned(size, 4)) return REN_ERR_BAD_ARG;
    const int64_t n = (int64_t)nx * ny * nz;
    const dim3 grid(ren_blocks(n, MC_THREADS)), block(MC_THREADS);
    hipLaunchKernelGGL(mesh_components_init_kernel, grid, block, 0, (hipStream_t)stream, sigma, (uint32_t)n, level, outside, label,
                       size, border);
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) {
        hipLaunchKernelGGL(mesh_components_union_kernel, grid, block, 0, (hipStream_t)stream, sigma, nx, ny, nz, level, outside,
                           label);
        e = hipGetLastError();
    }
    if (e != hipSuccess) {
        fprintf(stderr, "[ren_amd] %s:%d launch error: %s\n", __FILE__, __LINE__, hipGetErrorString(e));
        return REN_ERR_LAUNCH;
    }
    hipLaunchKernelGGL(mesh_components_flatten_kernel, grid, block, 0, (hipStream_t)stream, nx, ny, nz, label, size, border);
    REN_CHECK_LAUNCH();
}

extern "C" int ren_mesh_component_apply(const float *sigma, const int32_t *label, const uint8_t *drop, int64_t n, float value,
                                        float *out, void *stream) {
    if (n < 0 || n > REN_MESH_MAX_POINTS || value != value) return REN_ERR_BAD_ARG;
    if (!sigma || !label || !drop || !out) return REN_ERR_BAD_ARG;
    if (mc_misaligned(sigma, 4) || mc_misaligned(label, 4) || mc_misaligned(out, 4)) return REN_ERR_BAD_ARG;
    if (n == 0) return REN_OK;
    uint32_t bits;
    memcpy(&bits, &value, 4);
    hipLaunchKernelGGL(mesh_component_apply_kernel, dim3(ren_blocks(n, MC_THREADS)), dim3(MC_THREADS), 0, (hipStream_t)stream,
                       (const uint32_t *)sigma, label, drop, n, bits, (uint32_t *)out);
    REN_CHECK_LAUNCH();
}
