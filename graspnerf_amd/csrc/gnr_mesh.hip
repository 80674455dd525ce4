// Surface mesh of a scalar volume on the device: naive surface nets over the iso-surface vol = iso, one vertex per sign-changing
// cell and one quad (two triangles) per sign-changing interior voxel edge, as an indexed triangle mesh.  No reference counterpart
// (the reference hands its volume to Open3D on the host); the statement is include/gnr.h's and tests/mesh_reference.py's.
// Two ordered compactions like gnr_post.hip's surface cloud (gnr_compact.h: count per chunk of 1024 -> scan per scene -> write): the
// cells in ascending linear index, then the voxels' edges in ascending (voxel index * 3 + axis); the vertex pass leaves a
// cell -> vertex map in the workspace and the face pass looks the four cells of a quad up in it.  Nothing is atomic, every output row
// has a defined position: the result is a pure function of the input bits.
// The crossing parameters, the means and the frame change are float64, every operation one correctly rounded IEEE operation in the
// order written here (contraction is off for the whole file, as in gnr_tsdf.hip): the results are the bits of the numpy statement.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "gnr_compact.h"
#include "gnr_host.h"

#pragma clang fp contract(off)

namespace gnr_mesh {

using namespace gnr;

// the inside bits of a cell's corners, corner (dx,dy,dz) at bit dx*4 + dy*2 + dz, and their values
__device__ inline unsigned cell_corners(const float* __restrict__ vol, int R, int x, int y, int z, float iso, float (&c)[8]) {
    unsigned m = 0;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        c[k] = vol[((size_t)(x + (k >> 2)) * R + (size_t)(y + ((k >> 1) & 1))) * R + (size_t)(z + (k & 1))];
        m |= (c[k] < iso ? 1u : 0u) << k;
    }
    return m;
}

// cells: C = R - 1 per axis, nc = C^3 per scene, z fastest;  launch grid (chunks per scene, B)
__global__ __launch_bounds__(1024) void k_mesh_count_cells(const float* __restrict__ vol, int R, float iso, int* __restrict__ chunk) {
    __shared__ int wave_tot[16];
    const unsigned C = (unsigned)R - 1u, nc = C * C * C;               // R <= 256: nc < 2^24
    const unsigned t = blockIdx.x * 1024u + threadIdx.x;
    bool f[1] = {false};
    if (t < nc) {
        float c[8];
        const unsigned m = cell_corners(vol + (size_t)blockIdx.y * R * R * R, R, (int)(t / (C * C)), (int)((t / C) % C), (int)(t % C), iso, c);
        f[0] = m != 0u && m != 255u;
    }
    int tot;
    block_rank(f, wave_tot, tot);
    if (threadIdx.x == 0) chunk[(size_t)blockIdx.y * gridDim.x + blockIdx.x] = tot;
}

// the three edges (p, a) from voxel p = (x,y,z) towards +a that are interior and change sign;  returns whether p is inside
__device__ inline bool voxel_edges(const float* __restrict__ vol, int R, int x, int y, int z, float iso, bool (&f)[3]) {
    const size_t lin = ((size_t)x * R + y) * R + z;
    const bool in0 = vol[lin] < iso;
    const bool mx = x >= 1 && x <= R - 2, my = y >= 1 && y <= R - 2, mz = z >= 1 && z <= R - 2;      // strictly inside along the axis
    f[0] = x <= R - 2 && my && mz && (vol[lin + (size_t)R * R] < iso) != in0;
    f[1] = y <= R - 2 && mz && mx && (vol[lin + R] < iso) != in0;
    f[2] = z <= R - 2 && mx && my && (vol[lin + 1] < iso) != in0;
    return in0;
}

// voxels: n = R^3 per scene, z fastest;  launch grid (chunks per scene, B)
__global__ __launch_bounds__(1024) void k_mesh_count_edges(const float* __restrict__ vol, int R, float iso, int* __restrict__ chunk) {
    __shared__ int wave_tot[16];
    const unsigned Ru = (unsigned)R, n = Ru * Ru * Ru;                 // R <= 256: n <= 2^24
    const unsigned t = blockIdx.x * 1024u + threadIdx.x;
    bool f[3] = {false, false, false};
    if (t < n) voxel_edges(vol + (size_t)blockIdx.y * n, R, (int)(t / (Ru * Ru)), (int)((t / Ru) % Ru), (int)(t % Ru), iso, f);
    int tot;
    block_rank(f, wave_tot, tot);
    if (threadIdx.x == 0) chunk[(size_t)blockIdx.y * gridDim.x + blockIdx.x] = tot;
}

// exclusive scan of a scene's chunk counts in place, both compactions in one launch: grid (B, 2), y = 0 the cells (count[b][0] =
// vertices), y = 1 the edges (count[b][1] = 2 triangles per quad)
__global__ __launch_bounds__(1024) void k_mesh_scan(int* __restrict__ chunk_v, int nc_v, int* __restrict__ chunk_f, int nc_f, int* __restrict__ count) {
    __shared__ int wave_tot[16];
    const int which = blockIdx.y, nc = which ? nc_f : nc_v;
    const int total = scan_chunks((which ? chunk_f : chunk_v) + (size_t)blockIdx.x * nc, nc, wave_tot);
    if (threadIdx.x == 0) count[(size_t)blockIdx.x * 2 + which] = which ? 2 * total : total;
}

struct Frame { float iso; double scale, origin[3]; };

// The vertex of every active cell: the mean of the crossing points of its sign-changing edges, the 12 edges in the order
// a = 0,1,2; dc = 0,1; db = 0,1 (b = a+1, c = a+2 mod 3), summed sequentially per component.  map[cell] = the vertex's row, also
// beyond max_v (the faces name the true rows).
__global__ __launch_bounds__(1024) void k_mesh_vertices(const float* __restrict__ vol, const float* __restrict__ grad, int R, Frame fr,
                                                        const int* __restrict__ chunk, int max_v, int* __restrict__ map,
                                                        double* __restrict__ vertices, float* __restrict__ gradient) {
    __shared__ int wave_tot[16];
    const int b = blockIdx.y;
    const unsigned C = (unsigned)R - 1u, nc = C * C * C;
    const size_t n = (size_t)R * R * R;
    const unsigned t = blockIdx.x * 1024u + threadIdx.x;
    const int q[3] = {(int)(t / (C * C)), (int)((t / C) % C), (int)(t % C)};
    float c[8];
    unsigned m = 0;
    if (t < nc) m = cell_corners(vol + (size_t)b * n, R, q[0], q[1], q[2], fr.iso, c);
    const bool f[1] = {m != 0u && m != 255u};
    int tot;
    const int pos = chunk[(size_t)b * gridDim.x + blockIdx.x] + block_rank(f, wave_tot, tot);
    if (!f[0]) return;
    map[(size_t)b * nc + t] = pos;
    if (pos >= max_v) return;
    const double iso = (double)fr.iso;
    double s[3] = {0.0, 0.0, 0.0}, gs[3] = {0.0, 0.0, 0.0};
    int cnt = 0;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const int bb = (a + 1) % 3, cc = (a + 2) % 3;
#pragma unroll
        for (int dc = 0; dc < 2; ++dc) {
#pragma unroll
            for (int db = 0; db < 2; ++db) {
                const int k0 = (db << (2 - bb)) | (dc << (2 - cc)), k1 = k0 | (1 << (2 - a));      // corner bits: axis 0 -> 4, 1 -> 2, 2 -> 1
                if (((m >> k0) & 1u) == ((m >> k1) & 1u)) continue;
                const double v0 = (double)c[k0], v1 = (double)c[k1];
                const double tt = (iso - v0) / (v1 - v0);
                int p0[3] = {q[0], q[1], q[2]};
                p0[bb] += db; p0[cc] += dc;
#pragma unroll
                for (int k = 0; k < 3; ++k) s[k] += k == a ? (double)p0[k] + tt : (double)p0[k];
                ++cnt;
                if (grad) {
                    const float* g0 = grad + ((size_t)b * n + ((size_t)p0[0] * R + p0[1]) * R + p0[2]) * 3;
                    const float* g1 = g0 + (a == 0 ? (size_t)R * R : a == 1 ? (size_t)R : (size_t)1) * 3;
#pragma unroll
                    for (int k = 0; k < 3; ++k) {
                        const double a0 = (double)g0[k], a1 = (double)g1[k];
                        gs[k] += a0 + tt * (a1 - a0);
                    }
                }
            }
        }
    }
    const size_t o = ((size_t)b * max_v + pos) * 3;
    const double nn = (double)cnt;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const double mean = s[k] / nn;
        vertices[o + k] = fr.origin[k] + mean * fr.scale;
        if (grad) gradient[o + k] = (float)(gs[k] / nn);
    }
}

// The quad of every sign-changing interior edge (p, a), over the four cells around it by minimum corner q0 = p - e_b - e_c,
// q1 = p - e_c, q2 = p, q3 = p - e_b: (q0,q1,q2), (q0,q2,q3) when p is inside (vol rises along +a), else (q0,q2,q1), (q0,q3,q2);
// rows 2r and 2r + 1 of the r-th edge in (voxel index * 3 + a) order.  All four cells hold the edge, so they are active and mapped.
__global__ __launch_bounds__(1024) void k_mesh_faces(const float* __restrict__ vol, int R, float iso, const int* __restrict__ chunk,
                                                     const int* __restrict__ map, int max_f, int* __restrict__ faces) {
    __shared__ int wave_tot[16];
    const int b = blockIdx.y;
    const unsigned Ru = (unsigned)R, n = Ru * Ru * Ru;
    const int C = R - 1;
    const unsigned t = blockIdx.x * 1024u + threadIdx.x;
    const int p[3] = {(int)(t / (Ru * Ru)), (int)((t / Ru) % Ru), (int)(t % Ru)};
    bool f[3] = {false, false, false};
    bool in0 = false;
    if (t < n) in0 = voxel_edges(vol + (size_t)b * n, R, p[0], p[1], p[2], iso, f);
    int tot;
    int pos = chunk[(size_t)b * gridDim.x + blockIdx.x] + block_rank(f, wave_tot, tot);
    const int* mp = map + (size_t)b * C * C * C;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        if (!f[a]) continue;
        const int bb = (a + 1) % 3, cc = (a + 2) % 3;
        int q[4][3];
#pragma unroll
        for (int j = 0; j < 4; ++j) { q[j][0] = p[0]; q[j][1] = p[1]; q[j][2] = p[2]; }
        q[0][bb] -= 1; q[0][cc] -= 1; q[1][cc] -= 1; q[3][bb] -= 1;
        int v[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = mp[((size_t)q[j][0] * C + q[j][1]) * C + q[j][2]];
        const long long row = 2ll * pos;
        int* o = faces + ((size_t)b * max_f + (size_t)row) * 3;
        if (row < max_f) { o[0] = v[0]; o[1] = in0 ? v[1] : v[2]; o[2] = in0 ? v[2] : v[1]; }
        if (row + 1 < max_f) { o[3] = v[0]; o[4] = in0 ? v[2] : v[3]; o[5] = in0 ? v[3] : v[2]; }
        ++pos;
    }
}

static inline size_t chunks(size_t items) { return (items + 1023) / 1024; }

}  // namespace gnr_mesh

using namespace gnr_mesh;

// workspace: the cells' chunk counts [B, chunks((R-1)^3)], the edges' [B, chunks(R^3)], the cell -> vertex map [B, (R-1)^3], ints
struct MeshWork { int *chunk_v, *chunk_f, *map; size_t total; };

static MeshWork carve(int B, int R, void* base) {
    const size_t nc = (size_t)(R - 1) * (R - 1) * (R - 1), n = (size_t)R * R * R;
    Carve c(base);
    return MeshWork{c.take<int>(B * chunks(nc)), c.take<int>(B * chunks(n)), c.take<int>(B * nc), c.total()};     // (in this order)
}

extern "C" size_t gnr_surface_mesh_workspace_bytes(int B, int R) {
    return scenes_ok(B) && lattice_ok(R) ? carve(B, R, nullptr).total : 0;
}

extern "C" int gnr_surface_mesh_fwd(const float* vol, const float* grad, int B, int R, const GnrMeshParams* p, int* count, double* vertices,
                                    int* faces, float* gradient, int max_v, int max_f, void* ws, size_t ws_bytes, void* stream) {
    const Refuse no{"gnr_surface_mesh_fwd"};
    if (!vol || !p || !count || !vertices || !faces || !ws) return no(GNR_ERR_ARG, "null pointer");
    if ((grad == nullptr) != (gradient == nullptr)) return no(GNR_ERR_ARG, "grad and gradient must be both given or both NULL");
    if (int rc = check_scenes(no, GNR_ERR_SHAPE, B)) return rc;
    if (int rc = check_lattice(no, GNR_ERR_SHAPE, R)) return rc;
    if (max_v < 1) return no(GNR_ERR_SHAPE, "max_v must be >= 1");
    if (max_f < 1) return no(GNR_ERR_SHAPE, "max_f must be >= 1");
    if (!isfinite(p->iso) || !isfinite(p->scale) || !isfinite(p->origin[0]) || !isfinite(p->origin[1]) || !isfinite(p->origin[2]))
        return no(GNR_ERR_ARG, "iso, scale and origin must be finite");
    const MeshWork k = carve(B, R, ws);
    if (ws_bytes < k.total) return no(GNR_ERR_WORKSPACE, "workspace smaller than gnr_surface_mesh_workspace_bytes(B, R)");
    hipStream_t st = (hipStream_t)stream;
    const size_t nc = (size_t)(R - 1) * (R - 1) * (R - 1), n = (size_t)R * R * R;
    const int ch_v = (int)chunks(nc), ch_f = (int)chunks(n);
    int *chunk_v = k.chunk_v, *chunk_f = k.chunk_f, *map = k.map;
    const Frame fr{p->iso, p->scale, {p->origin[0], p->origin[1], p->origin[2]}};
    const dim3 grid_v(ch_v, B), grid_f(ch_f, B), block(1024);
    if (int rc = launch<k_mesh_count_cells>("k_mesh_count_cells@gnr_surface_mesh_fwd", st, grid_v, block, 0, vol, R, p->iso, chunk_v)) return rc;
    if (int rc = launch<k_mesh_count_edges>("k_mesh_count_edges@gnr_surface_mesh_fwd", st, grid_f, block, 0, vol, R, p->iso, chunk_f)) return rc;
    if (int rc = launch<k_mesh_scan>("k_mesh_scan@gnr_surface_mesh_fwd", st, dim3(B, 2), block, 0, chunk_v, ch_v, chunk_f, ch_f, count)) return rc;
    if (int rc = launch<k_mesh_vertices>("k_mesh_vertices@gnr_surface_mesh_fwd", st, grid_v, block, 0, vol, grad, R, fr, (const int*)chunk_v, max_v,
                                         map, vertices, gradient))
        return rc;
    return launch<k_mesh_faces>("k_mesh_faces@gnr_surface_mesh_fwd", st, grid_f, block, 0, vol, R, p->iso, (const int*)chunk_f, (const int*)map, max_f,
                                faces);
}
