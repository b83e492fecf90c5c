// Level-set mesh (include/ren_amd.h "mesh"): marching tetrahedra over a regular lattice of densities, with every index fixed
// by the lattice so that neither an edge -> vertex table nor an atomic is needed.
//
// A lattice point p = (i * ny + j) * nz + k is inside when sigma[p] >= level.  The cube based at p has the corners p + c for
// the corner codes c = dx | dy << 1 | dz << 2, and is cut into the six Kuhn tetrahedra (0, A, A | B, 7) with A = 1 << a,
// B = 1 << b for the permutations (a, b, c) of the axes in lexicographic order; all six share the diagonal 0 - 7.  Every
// tetrahedron edge runs from its lower-numbered vertex in one of the seven forward directions e = 0 .. 6 (codes 1, 2, 4, 3, 5,
// 6, 7), and that vertex owns it.  mask[p] holds the owned edges whose ends differ; the mesh vertex on edge (p, e) has the id
// voff[p] + popcount(mask[p] & ((1 << e) - 1)) with voff the exclusive scan of popcount(mask) -- the caller's scan.
//
// Kernel 1, mesh_classify_kernel: one lattice point per lane.  8 loads of sigma (its own and the seven forward neighbours,
// each range-checked; the k + 1 neighbours are the next lane's words, the others lie in the next row / slab and are shared
// with the lanes that own them: 4 B per point from memory), writes mask (1 B), vcount (4 B) and, where the point is the base
// of a cube, fcount (4 B) at the cube's index: per tetrahedron 0, 1 or 2 triangles for 0 | 4, 1 | 3 or 2 inside vertices.
//
// Kernel 2, mesh_write_kernel: one lattice point per lane again.  A lane whose mask is 0 owns no vertex, and its cube (all
// eight corners are reached from p by the seven directions, so mask[p] == 0 means they all agree with p) has no triangle: it
// reads its 1 B and leaves.  The others -- the surface, O(n^2) of the n^3 -- write their vertices in direction order and then
// the cube's triangles: the inside bits of the eight corners come from sigma[p] and mask[p] alone, the six other owners' mask
// and voff are loaded, and each of the six tetrahedra looks its inside set up in a 16-entry table of edge triples.  The
// orientation is combinatorial: a 16-bit table for the even permutations, inverted for the odd ones (the Kuhn tetrahedra of
// odd permutations are mirror images); the computed positions never enter, so triangles of zero area (sigma == level at
// lattice points) are indexed consistently with their neighbours.
//
// Vertex position, float32, every operation rounded on its own (this file is built with -ffp-contract=off):
//     t = (level - sigma_p) / (sigma_q - sigma_p), 0.5 when that is not finite;   u = float(i) + t * di (and j, k);
//     x = min(lo + u * h, hi)           (h = (hi - lo) / (n - 1) from the host; the min keeps the last lattice plane, where
//                                        the rounding of h and of u * h can overshoot hi by an ulp, inside the caller's box)
// No LDS, no atomics, no stack memory: all loops are unrolled over compile-time tables, the only run-time table is the
// read-only triangle table in global memory.
#include "ren_common.h"

namespace {

constexpr int MESH_THREADS = REN_MESH_THREADS;

// direction number of a corner code (nibble c; code 0 is the point itself) and corner code of a direction (nibble e)
constexpr uint32_t MESH_DIR_OF_CODE = 0x65423100u, MESH_CODE_OF_DIR = 0x7653421u;
// the tetrahedra's second and third corner codes (nibble t) and the odd permutations (bit t)
constexpr uint32_t MESH_TET_C1 = 0x442211u, MESH_TET_C2 = 0x656353u, MESH_TET_ODD = 0x26u;
// bit s: an even tetrahedron whose inside set is s (bit m = vertex m inside) lists its triangles clockwise seen from outside
constexpr uint32_t MESH_FLIP = 0x4D24u;
// triangles of the inside set s as 3-bit tetrahedron-edge numbers (01, 02, 03, 12, 13, 23 = 0 .. 5), three per triangle, lowest
// bits first.  One inside vertex a: the edges to the outside vertices in ascending order; three inside: the edges from the
// outside vertex likewise; two inside a < b, outside c < d: (ac, ad, bd), (ac, bd, bc).
__device__ const uint32_t MESH_TRI[16] = {0x0, 0x88, 0x118, 0x1c311, 0x159, 0x1d150, 0xd160, 0x162,
                                          0x162, 0x25148, 0x15158, 0x159, 0x14319, 0x118, 0x88, 0x0};

__device__ __forceinline__ constexpr int mesh_dir(int code) { return (int)(MESH_DIR_OF_CODE >> (4 * code) & 7u); }
__device__ __forceinline__ constexpr int mesh_code(int e) { return (int)(MESH_CODE_OF_DIR >> (4 * e) & 7u); }

struct mesh_f3 { float x, y, z; };

__global__ void __launch_bounds__(MESH_THREADS) mesh_classify_kernel(const float *__restrict__ sigma, int nx, int ny, int nz,
                                                                     float level, uint8_t *__restrict__ mask,
                                                                     int32_t *__restrict__ vcount, int32_t *__restrict__ fcount) {
    const uint32_t n = (uint32_t)nx * (uint32_t)ny * (uint32_t)nz;                  // <= 2^30 (checked by the host)
    const uint32_t p = blockIdx.x * (uint32_t)MESH_THREADS + threadIdx.x;
    if (p >= n) return;
    const uint32_t row = p / (uint32_t)nz;
    const int k = (int)(p - row * (uint32_t)nz), i = (int)(row / (uint32_t)ny), j = (int)(row - (uint32_t)i * (uint32_t)ny);
    const bool hx = i + 1 < nx, hy = j + 1 < ny, hz = k + 1 < nz;
    const int64_t sx = (int64_t)ny * nz, sy = nz;
    const bool in0 = sigma[p] >= level;                                             // NaN: outside
    uint32_t in8 = in0 ? 1u : 0u, m = 0;
#pragma unroll
    for (int e = 0; e < 7; ++e) {
        const int c = mesh_code(e);
        if ((!(c & 1) || hx) && (!(c & 2) || hy) && (!(c & 4) || hz)) {
            const bool inq = sigma[(int64_t)p + ((c & 1) ? sx : 0) + ((c & 2) ? sy : 0) + ((c & 4) ? 1 : 0)] >= level;
            in8 |= (inq ? 1u : 0u) << c;
            m |= (inq != in0 ? 1u : 0u) << e;
        }
    }
    mask[p] = (uint8_t)m;
    vcount[p] = __popc(m);
    if (hx && hy && hz) {
        int f = 0;
#pragma unroll
        for (int t = 0; t < 6; ++t) {
            const int c1 = (int)(MESH_TET_C1 >> (4 * t) & 7u), c2 = (int)(MESH_TET_C2 >> (4 * t) & 7u);
            const int inside = (int)((in8 & 1u) + (in8 >> c1 & 1u) + (in8 >> c2 & 1u) + (in8 >> 7 & 1u));
            f += inside == 2 ? 2 : ((inside == 1 || inside == 3) ? 1 : 0);
        }
        fcount[((int64_t)i * (ny - 1) + j) * (nz - 1) + k] = f;
    }
}

__device__ __forceinline__ int32_t mesh_pick(uint32_t n, int32_t e0, int32_t e1, int32_t e2, int32_t e3, int32_t e4, int32_t e5) {
    return n == 0 ? e0 : n == 1 ? e1 : n == 2 ? e2 : n == 3 ? e3 : n == 4 ? e4 : e5;
}

__global__ void __launch_bounds__(MESH_THREADS) mesh_write_kernel(const float *__restrict__ sigma, const uint8_t *__restrict__ mask,
                                                                  const int64_t *__restrict__ voff, const int64_t *__restrict__ foff,
                                                                  int nx, int ny, int nz, float level, mesh_f3 lo, mesh_f3 hi,
                                                                  mesh_f3 h, int64_t V, int64_t F, float *__restrict__ verts,
                                                                  int32_t *__restrict__ faces) {
    const uint32_t n = (uint32_t)nx * (uint32_t)ny * (uint32_t)nz;
    const uint32_t p = blockIdx.x * (uint32_t)MESH_THREADS + threadIdx.x;
    if (p >= n) return;
    const uint32_t m0 = mask[p] & 0x7Fu;
    if (m0 == 0) return;
    const uint32_t row = p / (uint32_t)nz;
    const int k = (int)(p - row * (uint32_t)nz), i = (int)(row / (uint32_t)ny), j = (int)(row - (uint32_t)i * (uint32_t)ny);
    const bool hx = i + 1 < nx, hy = j + 1 < ny, hz = k + 1 < nz;
    const int64_t sx = (int64_t)ny * nz, sy = nz;
    const float s0 = sigma[p];
    const bool in0 = s0 >= level;
    const int64_t v0 = voff[p];
    // ---- the vertices this point owns, in direction order
    int64_t v = v0;
#pragma unroll
    for (int e = 0; e < 7; ++e) {
        const int c = mesh_code(e);
        // a set bit of an edge that does not exist cannot come from mesh_classify_kernel; nothing is read for it regardless
        if ((m0 >> e & 1u) && (!(c & 1) || hx) && (!(c & 2) || hy) && (!(c & 4) || hz)) {
            const float sq = sigma[(int64_t)p + ((c & 1) ? sx : 0) + ((c & 2) ? sy : 0) + ((c & 4) ? 1 : 0)];
            float t = (level - s0) / (sq - s0);
            if (!(fabsf(t) <= 3.402823466e+38f)) t = 0.5f;                          // infinite or NaN
            const float ux = (float)i + t * (float)(c & 1), uy = (float)j + t * (float)(c >> 1 & 1),
                        uz = (float)k + t * (float)(c >> 2 & 1);
            if ((uint64_t)v < (uint64_t)V) {
                float *o = verts + 3 * v;
                o[0] = fminf(lo.x + ux * h.x, hi.x);
                o[1] = fminf(lo.y + uy * h.y, hi.y);
                o[2] = fminf(lo.z + uz * h.z, hi.z);
            }
            ++v;
        }
    }
    // ---- the triangles of the cube based here
    if (!(hx && hy && hz)) return;
    uint32_t in8 = in0 ? 1u : 0u;
#pragma unroll
    for (int c = 1; c < 8; ++c) in8 |= ((in0 ? 1u : 0u) ^ (m0 >> mesh_dir(c) & 1u)) << c;
    // mask and first vertex id of the owners: corners 0 .. 6 (corner 7 owns no edge of this cube)
    uint32_t mk[7];
    int32_t vo[7];
    mk[0] = m0;
    vo[0] = (int32_t)v0;
#pragma unroll
    for (int c = 1; c < 7; ++c) {
        const int64_t q = (int64_t)p + ((c & 1) ? sx : 0) + ((c & 2) ? sy : 0) + ((c & 4) ? 1 : 0);
        mk[c] = mask[q];
        vo[c] = (int32_t)voff[q];
    }
    int64_t f = foff[((int64_t)i * (ny - 1) + j) * (nz - 1) + k];
#pragma unroll
    for (int t = 0; t < 6; ++t) {
        const int c1 = (int)(MESH_TET_C1 >> (4 * t) & 7u), c2 = (int)(MESH_TET_C2 >> (4 * t) & 7u);
        const uint32_t s = (in8 & 1u) | (in8 >> c1 & 1u) << 1 | (in8 >> c2 & 1u) << 2 | (in8 >> 7 & 1u) << 3;
        if (s == 0 || s == 15) continue;
        const int32_t e01 = vo[0] + __popc(mk[0] & ((1u << mesh_dir(c1)) - 1u));
        const int32_t e02 = vo[0] + __popc(mk[0] & ((1u << mesh_dir(c2)) - 1u));
        const int32_t e03 = vo[0] + __popc(mk[0] & ((1u << mesh_dir(7)) - 1u));
        const int32_t e12 = vo[c1] + __popc(mk[c1] & ((1u << mesh_dir(c2 ^ c1)) - 1u));
        const int32_t e13 = vo[c1] + __popc(mk[c1] & ((1u << mesh_dir(7 ^ c1)) - 1u));
        const int32_t e23 = vo[c2] + __popc(mk[c2] & ((1u << mesh_dir(7 ^ c2)) - 1u));
        const bool flip = ((MESH_FLIP >> s ^ MESH_TET_ODD >> t) & 1u) != 0;
        uint32_t tri = MESH_TRI[s];
        const int n_tri = __popc(s) == 2 ? 2 : 1;
        for (int q = 0; q < n_tri; ++q) {
            const int32_t a = mesh_pick(tri & 7u, e01, e02, e03, e12, e13, e23);
            const int32_t b = mesh_pick(tri >> 3 & 7u, e01, e02, e03, e12, e13, e23);
            const int32_t c = mesh_pick(tri >> 6 & 7u, e01, e02, e03, e12, e13, e23);
            tri >>= 9;
            if ((uint64_t)f < (uint64_t)F) {
                int32_t *o = faces + 3 * f;
                o[0] = a;
                o[1] = flip ? c : b;
                o[2] = flip ? b : c;
            }
            ++f;
        }
    }
}

bool mesh_bad_lattice(int32_t nx, int32_t ny, int32_t nz) {
    return nx < 2 || ny < 2 || nz < 2 || (int64_t)nx * ny * nz > REN_MESH_MAX_POINTS;
}

bool mesh_misaligned(const void *p, uintptr_t bytes) { return ((uintptr_t)p & (bytes - 1)) != 0; }

}  // namespace

extern "C" int ren_mesh_classify(const float *sigma, int32_t nx, int32_t ny, int32_t nz, float level, uint8_t *mask,
                                 int32_t *vcount, int32_t *fcount, void *stream) {
    if (mesh_bad_lattice(nx, ny, nz) || level != level) return REN_ERR_BAD_ARG;
    if (!sigma || !mask || !vcount || !fcount) return REN_ERR_BAD_ARG;
    if (mesh_misaligned(sigma, 4) || mesh_misaligned(vcount, 4) || mesh_misaligned(fcount, 4)) return REN_ERR_BAD_ARG;
    const int64_t n = (int64_t)nx * ny * nz;
    hipLaunchKernelGGL(mesh_classify_kernel, dim3(ren_blocks(n, MESH_THREADS)), dim3(MESH_THREADS), 0, (hipStream_t)stream, sigma,
                       nx, ny, nz, level, mask, vcount, fcount);
    REN_CHECK_LAUNCH();
}

extern "C" int ren_mesh_write(const float *sigma, const uint8_t *mask, const int64_t *voff, const int64_t *foff, int32_t nx,
                              int32_t ny, int32_t nz, float level, const float *lo, const float *hi, const float *h, int64_t V,
                              int64_t F, float *verts, int32_t *faces, void *stream) {
    if (mesh_bad_lattice(nx, ny, nz) || level != level || V < 0 || F < 0) return REN_ERR_BAD_ARG;
    if (V > INT32_MAX) return REN_ERR_BAD_ARG;
    if (!sigma || !mask || !voff || !foff || !lo || !hi || !h) return REN_ERR_BAD_ARG;
    if ((V > 0 && !verts) || (F > 0 && !faces)) return REN_ERR_BAD_ARG;
    if (mesh_misaligned(sigma, 4) || mesh_misaligned(voff, 8) || mesh_misaligned(foff, 8) || mesh_misaligned(verts, 4) ||
        mesh_misaligned(faces, 4))
        return REN_ERR_BAD_ARG;
    for (int a = 0; a < 3; ++a)
        if (!(lo[a] < hi[a]) || !(h[a] > 0.f) || !(fabsf(lo[a]) <= 3.402823466e+38f) || !(fabsf(hi[a]) <= 3.402823466e+38f))
            return REN_ERR_BAD_ARG;
    if (V == 0 && F == 0) return REN_OK;
    const int64_t n = (int64_t)nx * ny * nz;
    const mesh_f3 l = {lo[0], lo[1], lo[2]}, u = {hi[0], hi[1], hi[2]}, s = {h[0], h[1], h[2]};
    hipLaunchKernelGGL(mesh_write_kernel, dim3(ren_blocks(n, MESH_THREADS)), dim3(MESH_THREADS), 0, (hipStream_t)stream, sigma, mask,
                       voff, foff, nx, ny, nz, level, l, u, s, V, F, verts, faces);
    REN_CHECK_LAUNCH();
}
