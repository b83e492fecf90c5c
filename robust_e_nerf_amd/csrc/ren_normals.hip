// Reverse-mode INPUT gradient of the grid encoding: dx[i] = sum_level sum_f dfeat[i, level, f] * d feat[i, level, f] / d x[i]
// (tcnn's grid backward-input; what a surface normal -grad(sigma) needs behind the density MLP's d sigma / d feat).
//
// One thread per sample, the levels in a loop inside it, three accumulators: every level's 8 corner entries are gathered ONCE
// (128 corner reads per sample, the encoder forward's gather and addresses: level_pos / corner_indices8 / gather_corners8) and
// contracted with the derivative of the trilinear weights -- +-scale on the differentiated axis times the other two weights,
// as in hashgrid_fwd_jvp_kernel.  No atomics, no LDS, nothing written but dx.  With a scene the unit-cube gradient goes through
// the transposed Jacobian of the contraction (the forward Jacobian is contract_jvp's), so dx is the world-space gradient.
#include "ren_hashgrid_common.h"

namespace {

// Transposed Jacobian of contract_jvp (ren_hashgrid_common.h): du, the gradient w.r.t. the unit-cube position, -> dxw, the
// gradient w.r.t. the world position x.  The unit position itself comes from contract_jvp (one source of truth for the
// cells); only the intermediates the Jacobian needs are formed again here.
__device__ __forceinline__ void contract_vjp(const ren_scene_dev &sc, const float *x, const float *du, float *dxw) {
    float y[3], dy[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) y[k] = (x[k] - sc.lo[k]) / (sc.hi[k] - sc.lo[k]);
    if (sc.ct == REN_CT_SPHERE) {
#pragma unroll
        for (int k = 0; k < 3; ++k) { y[k] = y[k] * 2.f - 1.f; dy[k] = du[k] * 0.25f; }
        const float m = sqrtf(y[0] * y[0] + y[1] * y[1] + y[2] * y[2]);
        if (m > 1.f) {
            // y' = y g(m): J = g I + (gp / m) y y^T, symmetric
            const float g = (2.f - 1.f / m) / m;
            const float gp = (-2.f + 2.f / m) / (m * m);
            const float yd = (y[0] * dy[0] + y[1] * dy[1] + y[2] * dy[2]) / m;
#pragma unroll
            for (int k = 0; k < 3; ++k) dy[k] = dy[k] * g + y[k] * gp * yd;
        }
#pragma unroll
        for (int k = 0; k < 3; ++k) dy[k] *= 2.f;
    } else if (sc.ct == REN_CT_TANH) {
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const float th = tanhf(y[k] - 0.5f);
            dy[k] = (1.f - th * th) * du[k] * 0.5f;
        }
    } else {
#pragma unroll
        for (int k = 0; k < 3; ++k) dy[k] = du[k];
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) dxw[k] = dy[k] / (sc.hi[k] - sc.lo[k]);
}

template <int LAYOUT, bool FROM_RAYS>
__global__ __launch_bounds__(256) void hashgrid_bwd_input_kernel(
    GridDev g, const float2 *__restrict__ table, const float *__restrict__ x_unit, ren_scene_dev sc,
    const float *__restrict__ rays_o, const float *__restrict__ rays_d, const int32_t *__restrict__ ray_indices,
    const float *__restrict__ t_starts, const float *__restrict__ t_ends, int64_t n, const float *__restrict__ dfeat,
    float *__restrict__ dx) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    float u[3], x[3] = {0.f, 0.f, 0.f};
    if (FROM_RAYS) {
        // midpoint and unit position by the tangent kernels' own functions (the tangent halves are unused and fold away):
        // the cells are those of ren_hashgrid_fwd_jvp for the same sample
        float xd[3], ud[3];
        sample_pos_jvp(rays_o, rays_d, rays_o, rays_d, ray_indices, t_starts, t_ends, i, x, xd);
        contract_jvp(sc, x, xd, u, ud);
    } else {
        u[0] = x_unit[3 * i]; u[1] = x_unit[3 * i + 1]; u[2] = x_unit[3 * i + 2];
    }
    float acc[3] = {0.f, 0.f, 0.f};
    const int64_t frag = (i >> 5) * (REN_MAX_LEVELS * 64) + (i & 31);
#pragma unroll 2
    for (int lvl = 0; lvl < g.n_levels; ++lvl) {
        float d0, d1;
        if (LAYOUT == 0) {
            const float2 d = reinterpret_cast<const float2 *>(dfeat)[i * g.n_levels + lvl];
            d0 = d.x; d1 = d.y;
        } else {
            d0 = dfeat[frag + lvl * 64];
            d1 = dfeat[frag + lvl * 64 + 32];
        }
        const float scale = g.scale[lvl];
        const LevelPos p = level_pos(u[0], u[1], u[2], scale);
        const float2 *tab = table + g.offset[lvl];
        float2 v[8];
        uint32_t idx[8];
        corner_indices8(p.c[0], p.c[1], p.c[2], g.res[lvl], g.size[lvl], g.hashed[lvl] != 0, idx);
        gather_corners8(tab, idx, v);
        float gx = 0.f, gy = 0.f, gz = 0.f;
#pragma unroll
        for (int c = 0; c < 8; ++c) {
            const float ax = (c & 1) ? p.w[0] : 1.f - p.w[0];
            const float ay = (c & 2) ? p.w[1] : 1.f - p.w[1];
            const float az = (c & 4) ? p.w[2] : 1.f - p.w[2];
            const float s = v[c].x * d0 + v[c].y * d1;            // corner entry . dfeat of this level
            const float sx = (c & 1) ? s : -s, sy = (c & 2) ? s : -s, sz = (c & 4) ? s : -s;
            gx += sx * (ay * az);
            gy += sy * (ax * az);
            gz += sz * (ax * ay);
        }
        acc[0] += scale * gx; acc[1] += scale * gy; acc[2] += scale * gz;
    }
    float out[3];
    if (FROM_RAYS) contract_vjp(sc, x, acc, out);
    else { out[0] = acc[0]; out[1] = acc[1]; out[2] = acc[2]; }
    dx[3 * i] = out[0]; dx[3 * i + 1] = out[1]; dx[3 * i + 2] = out[2];
}

}  // namespace

extern "C" int ren_hashgrid_bwd_input(const ren_grid_desc *grid, const float *table, const float *x_unit,
                                      const ren_scene_desc *scene, const float *rays_o, const float *rays_d,
                                      const int32_t *ray_indices, const float *t_starts, const float *t_ends,
                                      int64_t n, int32_t layout, const float *dfeat, float *dx, void *stream) {
    GridDev g;
    int rc = make_grid(grid, g);
    if (rc) return rc;
    if (!table || !dfeat || !dx || n < 0 || (layout != 0 && layout != 1)) return REN_ERR_BAD_ARG;
    const bool from_rays = x_unit == nullptr;
    if (from_rays && (!scene || !rays_o || !rays_d || !ray_indices || !t_starts || !t_ends)) return REN_ERR_BAD_ARG;
    if (layout == 1 && g.n_levels != REN_MAX_LEVELS) return REN_ERR_UNSUPPORTED;
    if (n == 0) return REN_OK;
    ren_scene_dev sc = {};
    if (from_rays) sc = ren_make_scene(scene);
    dim3 grd((unsigned)ren_blocks(n, 256)), blk(256);
    const float2 *tab = reinterpret_cast<const float2 *>(table);
#define LAUNCH(L, R)                                                                                              \
    hipLaunchKernelGGL((hashgrid_bwd_input_kernel<L, R>), grd, blk, 0, (hipStream_t)stream, g, tab, x_unit, sc,   \
                       rays_o, rays_d, ray_indices, t_starts, t_ends, n, dfeat, dx)
    if (layout == 0) { if (from_rays) LAUNCH(0, true); else LAUNCH(0, false); }
    else             { if (from_rays) LAUNCH(1, true); else LAUNCH(1, false); }
#undef LAUNCH
    REN_CHECK_LAUNCH();
}
