// Mesh simplification by vertex clustering (include/ren_amd.h "mesh simplify"): the vertices of a triangle list are gathered
// into the cells of a regular grid over the world box, every occupied cell becomes one vertex at the mean of its members, and
// the faces that collapse (two corners in one cell) or repeat (the same cells in the same orientation) are dropped.
//
// The mean is a quotient of INTEGER sums: each member adds its position within the cell, quantised to 2^-20 of the cell, to
// three uint64 sums and 1 to a uint32 count with integer atomic adds.  Integer addition commutes exactly, so the sums and with
// them every output bit are functions of the input alone, whatever order the atomics land in.  No floating-point atomic, no
// LDS, no stack memory; every real operation is float64 and rounded on its own (this file is built with -ffp-contract=off).
//
// Kernel 1, simplify_cells_kernel: one vertex per lane.  12 B read, its cell id written (4 B), four atomic adds (28 B).
// Kernel 2, simplify_flags_kernel: one cell per lane, flag = (count != 0) for the caller's exclusive scan: the provisional id
//   of an occupied cell is the number of occupied cells before it.
// Kernel 3, simplify_faces_kernel: one face per lane.  The three corner indices are range-checked BEFORE anything is gathered
//   through them; then cell[corner] and coff[cell] give the provisional ids.  A face with a corner out of range or two equal
//   ids is degenerate: ids -1, both key words at their maximum, so that it sorts behind every real face.  Otherwise the key
//   is the id triple rotated to start at its smallest id: key_a = that id, key_b = second << 31 | third.  The degenerate
//   faces of a wave are counted by one ballot and one integer atomic add.
// Between 3 and 4 the CALLER orders the faces by (key_a, key_b) with stable sorts: equal keys then stand next to each other
//   in ascending input index.
// Kernel 4, simplify_heads_kernel: one sorted position per lane.  The face there is kept when it is not degenerate and its key
//   differs from the key of the position before it -- the first of its run, that is the smallest input index.  A kept face
//   marks its three provisional ids as used: plain stores of the same word by every writer.
// Kernel 5, simplify_vertices_kernel: one cell per lane.  An occupied cell whose provisional id is used writes its
//   representative to its final row uoff[provisional id]: the representative write and the vertex compaction in one pass.
// Kernel 6, simplify_compact_faces_kernel: one face per lane.  A kept face writes uoff[id] of its own three corners, in its
//   own corner order, to row foff[face].
// Every index that comes out of memory is compared with the size of what it indexes before it is used.
#include "ren_common.h"

namespace {

constexpr int MS_THREADS = REN_MESH_THREADS;
constexpr double MS_Q_ONE = 1048576.0;                                              // 2^20 steps across one cell
constexpr int32_t MS_KEY_A_NONE = INT32_MAX;
constexpr int64_t MS_KEY_B_NONE = INT64_MAX;

struct ms_d3 { double x, y, z; };
struct ms_i3 { int32_t x, y, z; };

// cell coordinate and quantised offset of one coordinate: r = (double(x) - lo) * inv
__device__ __forceinline__ void ms_axis(float x, double lo, double inv, int32_t g, int32_t &c, unsigned long long &q) {
    const double r = ((double)x - lo) * inv;
    const double fl = floor(r);
    if (!(fl >= 0.0)) c = 0;                                                        // NaN lands here
    else if (fl >= (double)g) c = g - 1;
    else c = (int32_t)fl;
    double frac = r - (double)c;
    if (!(frac >= 0.0)) frac = 0.0;
    if (frac > 1.0) frac = 1.0;
    q = (unsigned long long)floor(frac * MS_Q_ONE + 0.5);                           // 0 .. 2^20
}

__global__ void __launch_bounds__(MS_THREADS) simplify_cells_kernel(const float *__restrict__ verts, int64_t V, ms_d3 lo, ms_d3 inv,
                                                                    ms_i3 g, int32_t *__restrict__ cell,
                                                                    unsigned long long *sums, uint32_t *count) {
    const int64_t v = (int64_t)blockIdx.x * MS_THREADS + threadIdx.x;
    if (v >= V) return;
    const float *x = verts + 3 * v;
    int32_t cx, cy, cz;
    unsigned long long qx, qy, qz;
    ms_axis(x[0], lo.x, inv.x, g.x, cx, qx);
    ms_axis(x[1], lo.y, inv.y, g.y, cy, qy);
    ms_axis(x[2], lo.z, inv.z, g.z, cz, qz);
    const int32_t c = (cx * g.y + cy) * g.z + cz;                                   // < gx gy gz <= 2^30
    cell[v] = c;
    atomicAdd(sums + 3 * (int64_t)c, qx);
    atomicAdd(sums + 3 * (int64_t)c + 1, qy);
    atomicAdd(sums + 3 * (int64_t)c + 2, qz);
    atomicAdd(count + c, 1u);
}

__global__ void __launch_bounds__(MS_THREADS) simplify_flags_kernel(const uint32_t *__restrict__ count, int64_t n_cells,
                                                                    int32_t *__restrict__ flag) {
    const int64_t c = (int64_t)blockIdx.x * MS_THREADS + threadIdx.x;
    if (c >= n_cells) return;
    flag[c] = count[c] != 0u ? 1 : 0;
}

__global__ void __launch_bounds__(MS_THREADS) simplify_faces_kernel(const int32_t *__restrict__ faces, int64_t F, int64_t V,
                                                                    const int32_t *__restrict__ cell, const int64_t *__restrict__ coff,
                                                                    int64_t n_cells, int64_t clusters, int32_t *__restrict__ ids,
                                                                    int32_t *__restrict__ key_a, int64_t *__restrict__ key_b,
                                                                    int32_t *degenerate) {
    const int64_t f = (int64_t)blockIdx.x * MS_THREADS + threadIdx.x;
    bool bad = false;
    if (f < F) {
        int32_t id[3];
        bad = false;
#pragma unroll
        for (int m = 0; m < 3; ++m) {
            const int32_t corner = faces[3 * f + m];
            id[m] = -1;
            if (corner >= 0 && (int64_t)corner < V) {                               // checked before the gather
                const int32_t c = cell[corner];
                if (c >= 0 && (int64_t)c < n_cells) {
                    const int64_t p = coff[c];
                    if (p >= 0 && p < clusters) id[m] = (int32_t)p;                 // clusters <= 2^30
                }
            }
            bad = bad || id[m] < 0;
        }
        bad = bad || id[0] == id[1] || id[1] == id[2] || id[0] == id[2];
        int32_t a = MS_KEY_A_NONE;
        int64_t b = MS_KEY_B_NONE;
        if (bad) {
            id[0] = id[1] = id[2] = -1;
        } else {                                                                    // rotate the smallest id to the front
            const bool first = id[0] < id[1] && id[0] < id[2], second = !first && id[1] < id[2];
            const int32_t k0 = first ? id[0] : second ? id[1] : id[2];
            const int32_t k1 = first ? id[1] : second ? id[2] : id[0];
            const int32_t k2 = first ? id[2] : second ? id[0] : id[1];
            a = k0;
            b = (int64_t)k1 << 31 | (int64_t)k2;
        }
        ids[3 * f] = id[0];
        ids[3 * f + 1] = id[1];
        ids[3 * f + 2] = id[2];
        key_a[f] = a;
        key_b[f] = b;
    }
    const unsigned long long all_bad = __ballot(bad);                               // one add per wave
    if (all_bad && (threadIdx.x & (REN_WAVE - 1)) == (unsigned)(__ffsll(all_bad) - 1)) atomicAdd(degenerate, (int32_t)__popcll(all_bad));
}

__global__ void __launch_bounds__(MS_THREADS) simplify_heads_kernel(const int64_t *__restrict__ order, const int32_t *__restrict__ key_a,
                                                                    const int64_t *__restrict__ key_b, const int32_t *__restrict__ ids,
                                                                    int64_t F, int64_t clusters, int32_t *__restrict__ keep,
                                                                    int32_t *used) {
    const int64_t i = (int64_t)blockIdx.x * MS_THREADS + threadIdx.x;
    if (i >= F) return;
    const int64_t f = order[i];
    if (f < 0 || f >= F) return;                                                    // not a permutation: nothing is written through it
    const int32_t a = key_a[f];
    const int64_t b = key_b[f];
    bool head = a != MS_KEY_A_NONE;
    if (head && i > 0) {
        const int64_t before = order[i - 1];
        if (before >= 0 && before < F) head = key_a[before] != a || key_b[before] != b;
    }
    keep[f] = head ? 1 : 0;
    if (!head) return;
#pragma unroll
    for (int m = 0; m < 3; ++m) {
        const int32_t id = ids[3 * f + m];
        if (id >= 0 && (int64_t)id < clusters) used[id] = 1;
    }
}

__global__ void __launch_bounds__(MS_THREADS) simplify_vertices_kernel(const unsigned long long *__restrict__ sums,
                                                                       const uint32_t *__restrict__ count,
                                                                       const int64_t *__restrict__ coff, const int32_t *__restrict__ used,
                                                                       const int64_t *__restrict__ uoff, ms_i3 g, ms_d3 lo, ms_d3 cw,
                                                                       int64_t clusters, int64_t V_out, float *__restrict__ verts) {
    const int64_t n_cells = (int64_t)g.x * g.y * g.z;
    const int64_t c = (int64_t)blockIdx.x * MS_THREADS + threadIdx.x;
    if (c >= n_cells) return;
    const uint32_t n = count[c];
    if (n == 0u) return;
    const int64_t p = coff[c];
    if (p < 0 || p >= clusters || used[p] == 0) return;
    const int64_t row = uoff[p];
    if (row < 0 || row >= V_out) return;
    const int64_t plane = c / g.z;
    const int32_t cz = (int32_t)(c - plane * g.z), cx = (int32_t)(plane / g.y), cy = (int32_t)(plane - (int64_t)cx * g.y);
    const double members = (double)n;
    const double mx = (double)sums[3 * c] / members / MS_Q_ONE, my = (double)sums[3 * c + 1] / members / MS_Q_ONE,
                 mz = (double)sums[3 * c + 2] / members / MS_Q_ONE;
    float *o = verts + 3 * row;
    o[0] = (float)(lo.x + ((double)cx + mx) * cw.x);
    o[1] = (float)(lo.y + ((double)cy + my) * cw.y);
    o[2] = (float)(lo.z + ((double)cz + mz) * cw.z);
}

__global__ void __launch_bounds__(MS_THREADS) simplify_compact_faces_kernel(const int32_t *__restrict__ ids, const int32_t *__restrict__ keep,
                                                                            const int64_t *__restrict__ foff, const int64_t *__restrict__ uoff,
                                                                            int64_t F, int64_t clusters, int64_t F_out,
                                                                            int32_t *__restrict__ faces) {
    const int64_t f = (int64_t)blockIdx.x * MS_THREADS + threadIdx.x;
    if (f >= F || keep[f] == 0) return;
    const int64_t row = foff[f];
    if (row < 0 || row >= F_out) return;
#pragma unroll
    for (int m = 0; m < 3; ++m) {
        const int32_t id = ids[3 * f + m];
        faces[3 * row + m] = (id >= 0 && (int64_t)id < clusters) ? (int32_t)uoff[id] : -1;
    }
}

bool ms_misaligned(const void *p, uintptr_t bytes) { return ((uintptr_t)p & (bytes - 1)) != 0; }

bool ms_bad_grid(int32_t gx, int32_t gy, int32_t gz) {
    return gx < 1 || gy < 1 || gz < 1 || (int64_t)gx * gy > REN_MESH_MAX_POINTS || (int64_t)gx * gy * gz > REN_MESH_MAX_POINTS;
}

bool ms_bad_box(const double *lo, const double *hi) {
    for (int a = 0; a < 3; ++a)
        if (!(lo[a] < hi[a]) || !(fabs(lo[a]) <= 1.7976931348623157e308) || !(fabs(hi[a]) <= 1.7976931348623157e308)) return true;
    return false;
}

bool ms_bad_count(int64_t n) { return n < 0 || n > (int64_t)INT32_MAX; }

}  // namespace

extern "C" int ren_mesh_simplify_cells(const float *verts, int64_t V, const double *lo, const double *hi, int32_t gx, int32_t gy,
                                       int32_t gz, int32_t *cell, uint64_t *sums, uint32_t *count, void *stream) {
    if (ms_bad_grid(gx, gy, gz) || ms_bad_count(V) || !lo || !hi || ms_bad_box(lo, hi)) return REN_ERR_BAD_ARG;
    if (!sums || !count || (V > 0 && (!verts || !cell))) return REN_ERR_BAD_ARG;
    if (ms_misaligned(verts, 4) || ms_misaligned(cell, 4) || ms_misaligned(sums, 8) || ms_misaligned(count, 4)) return REN_ERR_BAD_ARG;
    if (V == 0) return REN_OK;
    const ms_d3 l = {lo[0], lo[1], lo[2]};
    const ms_d3 inv = {(double)gx / (hi[0] - lo[0]), (double)gy / (hi[1] - lo[1]), (double)gz / (hi[2] - lo[2])};
    const ms_i3 g = {gx, gy, gz};
    hipLaunchKernelGGL(simplify_cells_kernel, dim3(ren_blocks(V, MS_THREADS)), dim3(MS_THREADS), 0, (hipStream_t)stream, verts, V, l,
                       inv, g, cell, (unsigned long long *)sums, count);
    REN_CHECK_LAUNCH();
}

extern "C" int ren_mesh_simplify_flags(const uint32_t *count, int64_t n_cells, int32_t *flag, void *stream) {
    if (n_cells < 1 || n_cells > REN_MESH_MAX_POINTS || !count || !flag) return REN_ERR_BAD_ARG;
    if (ms_misaligned(count, 4) || ms_misaligned(flag, 4)) return REN_ERR_BAD_ARG;
    hipLaunchKernelGGL(simplify_flags_kernel, dim3(ren_blocks(n_cells, MS_THREADS)), dim3(MS_THREADS), 0, (hipStream_t)stream, count,
                       n_cells, flag);
    REN_CHECK_LAUNCH();
}

extern "C" int ren_mesh_simplify_faces(const int32_t *faces, int64_t F, int64_t V, const int32_t *cell, const int64_t *coff,
                                       int64_t n_cells, int64_t clusters, int32_t *ids, int32_t *key_a, int64_t *key_b,
                                       int32_t *degenerate, void *stream) {
    if (ms_bad_count(F) || ms_bad_count(V) || n_cells < 1 || n_cells > REN_MESH_MAX_POINTS || clusters < 0 || clusters > n_cells)
        return REN_ERR_BAD_ARG;
    if (!coff || !degenerate || (V > 0 && !cell) || (F > 0 && (!faces || !ids || !key_a || !key_b))) return REN_ERR_BAD_ARG;
    if (ms_misaligned(faces, 4) || ms_misaligned(cell, 4) || ms_misaligned(coff, 8) || ms_misaligned(ids, 4) ||
        ms_misaligned(key_a, 4) || ms_misaligned(key_b, 8) || ms_misaligned(degenerate, 4))
        return REN_ERR_BAD_ARG;
    if (F == 0) return REN_OK;
    hipLaunchKernelGGL(simplify_faces_kernel, dim3(ren_blocks(F, MS_THREADS)), dim3(MS_THREADS), 0, (hipStream_t)stream, faces, F, V,
                       cell, coff, n_cells, clusters, ids, key_a, key_b, degenerate);
    REN_CHECK_LAUNCH();
}

extern "C" int ren_mesh_simplify_heads(const int64_t *order, const int32_t *key_a, const int64_t *key_b, const int32_t *ids,
                                       int64_t F, int64_t clusters, int32_t *keep, int32_t *used, void *stream) {
    if (ms_bad_count(F) || clusters < 0 || clusters > REN_MESH_MAX_POINTS) return REN_ERR_BAD_ARG;
    if (F > 0 && (!order || !key_a || !key_b || !ids || !keep)) return REN_ERR_BAD_ARG;
    if (clusters > 0 && !used) return REN_ERR_BAD_ARG;
    if (ms_misaligned(order, 8) || ms_misaligned(key_a, 4) || ms_misaligned(key_b, 8) || ms_misaligned(ids, 4) ||
        ms_misaligned(keep, 4) || ms_misaligned(used, 4))
        return REN_ERR_BAD_ARG;
    if (F == 0) return REN_OK;
    hipLaunchKernelGGL(simplify_heads_kernel, dim3(ren_blocks(F, MS_THREADS)), dim3(MS_THREADS), 0, (hipStream_t)stream, order, key_a,
                       key_b, ids, F, clusters, keep, used);
    REN_CHECK_LAUNCH();
}

extern "C" int ren_mesh_simplify_vertices(const uint64_t *sums, const uint32_t *count, const int64_t *coff, const int32_t *used,
                                          const int64_t *uoff, int32_t gx, int32_t gy, int32_t gz, const double *lo, const double *hi,
                                          int64_t clusters, int64_t V_out, float *verts, void *stream) {
    if (ms_bad_grid(gx, gy, gz) || !lo || !hi || ms_bad_box(lo, hi)) return REN_ERR_BAD_ARG;
    const int64_t n_cells = (int64_t)gx * gy * gz;
    if (clusters < 0 || clusters > n_cells || V_out < 0 || V_out > clusters) return REN_ERR_BAD_ARG;
    if (!sums || !count || !coff || (clusters > 0 && (!used || !uoff)) || (V_out > 0 && !verts)) return REN_ERR_BAD_ARG;
    if (ms_misaligned(sums, 8) || ms_misaligned(count, 4) || ms_misaligned(coff, 8) || ms_misaligned(used, 4) ||
        ms_misaligned(uoff, 8) || ms_misaligned(verts, 4))
        return REN_ERR_BAD_ARG;
    if (V_out == 0) return REN_OK;
    const ms_d3 l = {lo[0], lo[1], lo[2]};
    const ms_d3 cw = {(hi[0] - lo[0]) / (double)gx, (hi[1] - lo[1]) / (double)gy, (hi[2] - lo[2]) / (double)gz};
    const ms_i3 g = {gx, gy, gz};
    hipLaunchKernelGGL(simplify_vertices_kernel, dim3(ren_blocks(n_cells, MS_THREADS)), dim3(MS_THREADS), 0, (hipStream_t)stream,
                       (const unsigned long long *)sums, count, coff, used, uoff, g, l, cw, clusters, V_out, verts);
    REN_CHECK_LAUNCH();
}

extern "C" int ren_mesh_simplify_compact_faces(const int32_t *ids, const int32_t *keep, const int64_t *foff, const int64_t *uoff,
                                               int64_t F, int64_t clusters, int64_t F_out, int32_t *faces, void *stream) {
    if (ms_bad_count(F) || clusters < 0 || clusters > REN_MESH_MAX_POINTS || F_out < 0 || F_out > F) return REN_ERR_BAD_ARG;
    if (F > 0 && (!ids || !keep || !foff)) return REN_ERR_BAD_ARG;
    if ((clusters > 0 && !uoff) || (F_out > 0 && !faces)) return REN_ERR_BAD_ARG;
    if (ms_misaligned(ids, 4) || ms_misaligned(keep, 4) || ms_misaligned(foff, 8) || ms_misaligned(uoff, 8) || ms_misaligned(faces, 4))
        return REN_ERR_BAD_ARG;
    if (F_out == 0) return REN_OK;
    hipLaunchKernelGGL(simplify_compact_faces_kernel, dim3(ren_blocks(F, MS_THREADS)), dim3(MS_THREADS), 0, (hipStream_t)stream, ids,
                       keep, foff, uoff, F, clusters, F_out, faces);
    REN_CHECK_LAUNCH();
}
