// isosurface.hip — mesh export (gfx950, wave64): the points of a regular grid for the density query, and the iso-surface of a density
// volume by marching tetrahedra on the Kuhn split.  A translation unit of its own: plain HIP, no MLP kernel header, no other object
// changes with it.  The reference declares --mesh_only / --mesh_grid_size (models/options.py:69-70) and never reads them: there is no
// counterpart to cite beyond those two lines; include/dfnet_hip.h holds the specification.
//
// Node (i,j,k) has id = (i ny + j) nz + k (z fastest); a node is INSIDE iff sigma >= iso (fp32 compare, NaN outside).  A cell is split
// into 6 tetrahedra, one per permutation (a,b,c) of the axes in lexicographic order: v0 = (0,0,0), v1 = v0 + e_a, v2 = v1 + e_b,
// v3 = (1,1,1).  The split is the same in every cell, so neighbouring cells agree on their shared faces and the surface is watertight.
// Its edges leave a node in the 7 directions d in {0,1}^3 \ 0, type = dx + 2 dy + 4 dz - 1; a crossed edge (its ends differ in
// inside-ness) carries one vertex, and vertex ids are the ranks of the crossed edges in the order of key = id(lower node) 7 + type.
// Faces are ordered by cell, tet, triangle.  Nothing is appended with atomics: count -> exclusive scan -> emit, so the output is
// bit-reproducible.
//
//   count_kernel       one thread per node: the 7 crossing bits (1 byte), the cell's triangle count, and both counts scanned
//                      exclusively inside the block of kScan nodes (one packed wave64 shuffle scan); block totals beside them
//   scan_sums_kernel   ONE block: exclusive scan of the block totals in trips of kTop with a running carry, and the two grand totals
//   emit_kernel        one thread per node: a vertex per set bit, the triangles of its cell.  The add-back of the scanned block sums
//                      happens where a prefix is read (prefix[id] + sums[id / kScan]): no pass of its own over the prefix arrays
// Bytes that MUST move per node: count reads 4 B of sigma (its 7 other loads re-read neighbours' values: expected from cache, not
// measured with counters) and writes 9 B; emit reads 1 B (the bits) and touches the rest only where the surface is.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/dfnet_hip.h"
#include "dfn_common.h"

namespace dfn {
namespace iso {

// nodes per block of count_kernel = one scan block.  Two files repeat the value by hand and must follow a change of it: the large cases
// of tests/test_gpu_isosurface.py are sized by it, and tools/gpu_mesh_timing.py (SCAN_BLOCK) counts the bytes of the block sums with it
constexpr int kScan = 256;
constexpr int kTop = 1024;                      // block sums per trip of scan_sums_kernel
constexpr long long kMaxNodes = 178956970LL;    // 12 triangles per cell: 12 nodes < 2^31 keeps every 32-bit count, prefix and id exact

// ---------------------------------------------------------------------------------------------- the case table, built by the compiler
// permutations xyz, xzy, yxz, yzx, zxy, zyx: the first axis of tet 0..5 is 0 0 1 1 2 2, the second the smaller / larger of the other two
__host__ __device__ constexpr int tet_axis_a(int tet) { return tet >> 1; }
__host__ __device__ constexpr int tet_axis_b(int tet) { return (tet & 1) ? (tet >> 1 == 2 ? 1 : 2) : (tet >> 1 == 0 ? 1 : 0); }
// corner code of tet vertex v: bit 0 = +x, bit 1 = +y, bit 2 = +z.  The codes of a tet grow as sets, so the lower node of the tet edge
// (x, y), x < y, is vertex x and its type is (code y ^ code x) - 1
__host__ __device__ constexpr int tet_corner(int tet, int v) {
  return v == 0 ? 0 : v == 1 ? (1 << tet_axis_a(tet)) : v == 2 ? ((1 << tet_axis_a(tet)) | (1 << tet_axis_b(tet))) : 7;
}
constexpr int popc4(int m) { return (m & 1) + ((m >> 1) & 1) + ((m >> 2) & 1) + ((m >> 3) & 1); }
constexpr int low4(int m) { return (m & 1) ? 0 : (m & 2) ? 1 : (m & 4) ? 2 : 3; }
constexpr int high4(int m) { return (m & 8) ? 3 : (m & 4) ? 2 : (m & 2) ? 1 : 0; }
__host__ __device__ constexpr int tet_triangles(int m) {   // m: bit v = tet vertex v inside
  const int k = (m & 1) + ((m >> 1) & 1) + ((m >> 2) & 1) + ((m >> 3) & 1);
  return (k == 0 || k == 4) ? 0 : (k == 2 ? 2 : 1);
}

struct CaseTable { uint32_t tri[6][16][2]; };   // per (tet, inside mask, triangle): 3 x 6 bits = (type << 3 | lower corner code), wound
constexpr CaseTable make_case_table() {
  CaseTable T{};
  for (int tet = 0; tet < 6; ++tet)
    for (int m = 1; m < 15; ++m)
      for (int tri = 0; tri < tet_triangles(m); ++tri) {
        int ex[3] = {0, 0, 0}, ey[3] = {0, 0, 0};   // corner t of the triangle lies on the tet edge (ex[t], ey[t])
        if (popc4(m) == 2) {                        // inside p < q, outside r < s: quad A=(p,r) B=(p,s) C=(q,s) D=(q,r) as (A,B,C), (A,C,D)
          const int p = low4(m), q = high4(m), r = low4(~m & 15), s = high4(~m & 15);
          ex[0] = p, ey[0] = r;
          if (tri == 0) ex[1] = p, ey[1] = s, ex[2] = q, ey[2] = s;
          else ex[1] = q, ey[1] = s, ex[2] = q, ey[2] = r;
        } else {                                    // the odd vertex out w against the others in increasing order
          const int w = low4(popc4(m) == 1 ? m : (~m & 15));
          for (int j = 0; j < 3; ++j) ex[j] = w, ey[j] = j + (j >= w ? 1 : 0);
        }
        // winding on the unit cell with every crossing at the edge midpoint (coordinates doubled: integers): the normal must point
        // from the inside vertices to the outside ones
        int P[3][3] = {};
        for (int t = 0; t < 3; ++t)
          for (int c = 0; c < 3; ++c) P[t][c] = ((tet_corner(tet, ex[t]) >> c) & 1) + ((tet_corner(tet, ey[t]) >> c) & 1);
        const int u[3] = {P[1][0] - P[0][0], P[1][1] - P[0][1], P[1][2] - P[0][2]};
        const int v[3] = {P[2][0] - P[0][0], P[2][1] - P[0][1], P[2][2] - P[0][2]};
        const int nrm[3] = {u[1] * v[2] - u[2] * v[1], u[2] * v[0] - u[0] * v[2], u[0] * v[1] - u[1] * v[0]};
        const int kin = popc4(m), kout = 4 - kin;
        int dot = 0;   // (centroid of the outside vertices - centroid of the inside ones) kin kout . normal
        for (int c = 0; c < 3; ++c) {
          int in = 0, out = 0;
          for (int vtx = 0; vtx < 4; ++vtx) ((m >> vtx) & 1 ? in : out) += (tet_corner(tet, vtx) >> c) & 1;
          dot += (out * kin - in * kout) * nrm[c];
        }
        uint32_t code[3] = {};
        for (int t = 0; t < 3; ++t) {
          const int lo = ex[t] < ey[t] ? ex[t] : ey[t], hi = ex[t] < ey[t] ? ey[t] : ex[t];
          const int clo = tet_corner(tet, lo), type = (tet_corner(tet, hi) ^ clo) - 1;
          code[t] = (uint32_t)((type << 3) | clo);
        }
        T.tri[tet][m][tri] = dot > 0 ? (code[0] | code[1] << 6 | code[2] << 12) : (code[0] | code[2] << 6 | code[1] << 12);
      }
  return T;
}
__constant__ CaseTable kCases = make_case_table();

// ---------------------------------------------------------------------------------------------- workspace
struct Layout { size_t vpre, fpre, vsum, fsum, bits, total; };   // byte offsets: two uint32 [n], two uint32 [blocks], uint8 [n]
static Layout layout(size_t n) {
  const size_t nb = (n + kScan - 1) / kScan;
  auto up = [](size_t b) { return (b + 255) & ~(size_t)255; };
  Layout L;
  size_t o = 0;
  L.vpre = o, o += up(n * 4);
  L.fpre = o, o += up(n * 4);
  L.vsum = o, o += up(nb * 4);
  L.fsum = o, o += up(nb * 4);
  L.bits = o, o += up(n);
  L.total = o;
  return L;
}

struct Grid { int nx, ny, nz; uint32_t n, sx, sy; };   // sx = ny nz, sy = nz: node strides (the z stride is 1)
__device__ __forceinline__ uint32_t corner_offset(const Grid& g, int code) {
  return (code & 1 ? g.sx : 0u) + (code & 2 ? g.sy : 0u) + (uint32_t)(code >> 2);
}
__device__ __forceinline__ bool inside(float s, float iso) { return s >= iso; }   // NaN compares false: outside

// inclusive scan over the 64 lanes of a wave
__device__ __forceinline__ uint32_t wave_scan(uint32_t x) {
  const int lane = threadIdx.x & 63;
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const uint32_t y = __shfl_up(x, off, 64);
    if (lane >= off) x += y;
  }
  return x;
}

// ---------------------------------------------------------------------------------------------- grid points
__global__ __launch_bounds__(256) void grid_points_kernel(const float* __restrict__ xs, const float* __restrict__ ys,
                                                          const float* __restrict__ zs, int ny, int nz, int i0, size_t n_floats,
                                                          float* __restrict__ pts) {
  const size_t step = (size_t)gridDim.x * blockDim.x;
  for (size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x; e < n_floats; e += step) {   // one float per trip: coalesced stores
    const size_t p = e / 3;
    const int c = (int)(e - p * 3);
    const size_t row = p / (size_t)nz;
    const int k = (int)(p - row * nz);
    const size_t plane = row / (size_t)ny;
    const int j = (int)(row - plane * ny);
    pts[e] = c == 0 ? xs[i0 + (int)plane] : c == 1 ? ys[j] : zs[k];
  }
}

// ---------------------------------------------------------------------------------------------- count
__global__ __launch_bounds__(kScan) void count_kernel(const float* __restrict__ sigma, Grid g, float iso, uint32_t* __restrict__ vpre,
                                                      uint32_t* __restrict__ fpre, uint32_t* __restrict__ vsum,
                                                      uint32_t* __restrict__ fsum, uint8_t* __restrict__ bits_out) {
  const uint32_t id = blockIdx.x * (uint32_t)kScan + threadIdx.x;
  uint32_t nv = 0, nf = 0;
  if (id < g.n) {
    const int i = (int)(id / g.sx), rem = (int)(id - (uint32_t)i * g.sx), j = rem / g.nz, k = rem - j * g.nz;
    const bool in0 = inside(sigma[id], iso);
    const int ok = (i + 1 < g.nx ? 1 : 0) | (j + 1 < g.ny ? 2 : 0) | (k + 1 < g.nz ? 4 : 0);   // the axes with a node one step up
    uint32_t in8 = in0 ? 1u : 0u, bits = 0;
#pragma unroll
    for (int d = 1; d < 8; ++d)
      if ((ok & d) == d) {   // the neighbour id + d is a node of the grid: the edge exists
        const bool ind = inside(sigma[id + corner_offset(g, d)], iso);
        in8 |= (ind ? 1u : 0u) << d;
        bits |= (ind != in0 ? 1u : 0u) << (d - 1);
      }
    bits_out[id] = (uint8_t)bits;
    nv = __popc(bits);
    if (ok == 7) {           // the node is the lowest corner of a cell
#pragma unroll
      for (int tet = 0; tet < 6; ++tet) {
        const int m = (int)((in8 & 1u) | ((in8 >> tet_corner(tet, 1)) & 1u) << 1 | ((in8 >> tet_corner(tet, 2)) & 1u) << 2 | (in8 >> 7) << 3);
        nf += tet_triangles(m);
      }
    }
  }
  // exclusive scan of both counts over the block, packed: a block holds at most 256 x 7 vertices and 256 x 12 triangles
  const uint32_t x = nv | nf << 16;
  const uint32_t incl = wave_scan(x);
  __shared__ uint32_t wtot[kScan / 64];
  if ((threadIdx.x & 63) == 63) wtot[threadIdx.x >> 6] = incl;
  __syncthreads();
  uint32_t before = 0, total = 0;
#pragma unroll
  for (int w = 0; w < kScan / 64; ++w) {
    if (w < (int)(threadIdx.x >> 6)) before += wtot[w];
    total += wtot[w];
  }
  const uint32_t excl = before + incl - x;
  if (id < g.n) vpre[id] = excl & 0xffffu, fpre[id] = excl >> 16;
  if (threadIdx.x == 0) vsum[blockIdx.x] = total & 0xffffu, fsum[blockIdx.x] = total >> 16;
}

// ONE block: the block totals become exclusive prefixes in place; totals[0..1] = V, F
__global__ __launch_bounds__(kTop) void scan_sums_kernel(uint32_t* __restrict__ vsum, uint32_t* __restrict__ fsum, uint32_t nb,
                                                         unsigned long long* __restrict__ totals) {
  __shared__ uint32_t wv[kTop / 64], wf[kTop / 64];
  uint32_t carry_v = 0, carry_f = 0;   // the same in every thread
  for (uint32_t base = 0; base < nb; base += kTop) {
    const uint32_t i = base + threadIdx.x;
    const uint32_t xv = i < nb ? vsum[i] : 0u, xf = i < nb ? fsum[i] : 0u;
    const uint32_t iv = wave_scan(xv), jf = wave_scan(xf);
    if ((threadIdx.x & 63) == 63) wv[threadIdx.x >> 6] = iv, wf[threadIdx.x >> 6] = jf;
    __syncthreads();
    uint32_t bv = 0, bf = 0, tv = 0, tf = 0;
#pragma unroll
    for (int w = 0; w < kTop / 64; ++w) {
      if (w < (int)(threadIdx.x >> 6)) bv += wv[w], bf += wf[w];
      tv += wv[w], tf += wf[w];
    }
    if (i < nb) vsum[i] = carry_v + bv + iv - xv, fsum[i] = carry_f + bf + jf - xf;
    carry_v += tv, carry_f += tf;
    __syncthreads();   // wv / wf are rewritten by the next trip
  }
  if (threadIdx.x == 0) totals[0] = carry_v, totals[1] = carry_f;
}

// ---------------------------------------------------------------------------------------------- emit
struct Prefix { const uint32_t *vpre, *fpre, *vsum, *fsum; const uint8_t* bits; };
// the id of the vertex on the edge of `type` that leaves node `lo`
__device__ __forceinline__ uint32_t vertex_id(const Prefix& p, uint32_t lo, int type) {
  return p.vpre[lo] + p.vsum[lo / kScan] + __popc((uint32_t)p.bits[lo] & ((1u << type) - 1u));
}

__global__ __launch_bounds__(256) void emit_kernel(const float* __restrict__ sigma, const float* __restrict__ xs,
                                                   const float* __restrict__ ys, const float* __restrict__ zs, Grid g, float iso,
                                                   Prefix p, float* __restrict__ verts, uint32_t V, int* __restrict__ faces, uint32_t F) {
  const uint32_t id = blockIdx.x * 256u + threadIdx.x;
  if (id >= g.n) return;
  const uint32_t bits = p.bits[id] & 0x7fu;
  if (bits == 0) return;   // no crossed edge leaves the node, and every corner of its cell is on its side: nothing to write
  const int i = (int)(id / g.sx), rem = (int)(id - (uint32_t)i * g.sx), j = rem / g.nz, k = rem - j * g.nz;
  const int ok = (i + 1 < g.nx ? 1 : 0) | (j + 1 < g.ny ? 2 : 0) | (k + 1 < g.nz ? 4 : 0);
  const float s_a = sigma[id];
  // vertices: every read is of a node of the grid and every store below V, whatever the workspace holds
  uint32_t vid = p.vpre[id] + p.vsum[id / kScan];
  const float pa[3] = {xs[i], ys[j], zs[k]};
#pragma unroll
  for (int d = 1; d < 8; ++d) {
    if (!((bits >> (d - 1)) & 1u)) continue;
    if ((ok & d) == d && vid < V) {
      const float s_b = sigma[id + corner_offset(g, d)];
      const float pb[3] = {d & 1 ? xs[i + 1] : pa[0], d & 2 ? ys[j + 1] : pa[1], d & 4 ? zs[k + 1] : pa[2]};
      // t = clamp((iso - s_a) / (s_b - s_a), 0, 1), every operation rounded on its own; a NaN quotient clamps to 0 (fmaxf returns the number)
      const float t = fminf(fmaxf(__fdiv_rn(__fsub_rn(iso, s_a), __fsub_rn(s_b, s_a)), 0.f), 1.f);
#pragma unroll
      for (int c = 0; c < 3; ++c) verts[(size_t)vid * 3 + c] = __fadd_rn(pa[c], __fmul_rn(t, __fsub_rn(pb[c], pa[c])));
    }
    ++vid;
  }
  if (ok != 7) return;
  // triangles of the cell: the corners' sides from the node's own side and its crossing bits
  const uint32_t in8 = ((bits << 1) ^ (inside(s_a, iso) ? 0xffu : 0u)) & 0xffu;
  uint32_t f = p.fpre[id] + p.fsum[id / kScan];
#pragma unroll
  for (int tet = 0; tet < 6; ++tet) {
    const int m = (int)((in8 & 1u) | ((in8 >> tet_corner(tet, 1)) & 1u) << 1 | ((in8 >> tet_corner(tet, 2)) & 1u) << 2 | (in8 >> 7) << 3);
    const int nt = tet_triangles(m);
    for (int tri = 0; tri < nt; ++tri, ++f) {
      if (f >= F) continue;
      const uint32_t code = kCases.tri[tet][m][tri];
#pragma unroll
      for (int t = 0; t < 3; ++t) {
        const uint32_t c = code >> (6 * t);
        faces[(size_t)f * 3 + t] = (int)vertex_id(p, id + corner_offset(g, (int)(c & 7u)), (int)((c >> 3) & 7u));
      }
    }
  }
}

// argument rules shared by the entries: DFN_OK, or the status with the message set
static int check_dims(const char* who, int nx, int ny, int nz) {
  if (nx < 2 || ny < 2 || nz < 2) return set_error(DFN_ERR_ARG, "%s: nx, ny, nz must be >= 2 (got %d, %d, %d)", who, nx, ny, nz);
  if ((long long)nx * ny * nz > kMaxNodes)
    return set_error(DFN_ERR_UNSUPPORTED, "%s: %lld nodes, at most %lld (12 triangles per cell in 32-bit counts)", who,
                     (long long)nx * ny * nz, kMaxNodes);
  return DFN_OK;
}
static Grid make_grid(int nx, int ny, int nz) {
  Grid g;
  g.nx = nx, g.ny = ny, g.nz = nz;
  g.n = (uint32_t)((long long)nx * ny * nz), g.sx = (uint32_t)ny * (uint32_t)nz, g.sy = (uint32_t)nz;
  return g;
}

}  // namespace iso
}  // namespace dfn

extern "C" size_t dfn_isosurface_workspace_bytes(int nx, int ny, int nz) {
  using namespace dfn::iso;
  if (check_dims("dfn_isosurface_workspace_bytes", nx, ny, nz) != DFN_OK) return 0;
  return layout((size_t)nx * ny * nz).total;
}

extern "C" int dfn_grid_points(const float* xs, const float* ys, const float* zs, int nx, int ny, int nz, int i0, int i1, float* pts,
                               void* stream) {
  using namespace dfn;
  using namespace dfn::iso;
  if (const int rc = check_dims("dfn_grid_points", nx, ny, nz)) return rc;
  if (i0 < 0 || i1 < i0 || i1 > nx) return set_error(DFN_ERR_ARG, "dfn_grid_points: planes [%d, %d) outside 0..%d", i0, i1, nx);
  if (!xs || !ys || !zs || (!pts && i1 > i0)) return set_error(DFN_ERR_ARG, "dfn_grid_points: null pointer");
  if (i0 == i1) return DFN_OK;
  const size_t n_floats = (size_t)(i1 - i0) * ny * nz * 3;
  const size_t blocks = (n_floats + 255) / 256;
  hipLaunchKernelGGL(grid_points_kernel, dim3((unsigned)(blocks < 65536 ? blocks : 65536)), dim3(256), 0, static_cast<hipStream_t>(stream),
                     xs, ys, zs, ny, nz, i0, n_floats, pts);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return set_error(DFN_ERR_HIP, "dfn_grid_points: %s", hipGetErrorString(e));
  return DFN_OK;
}

extern "C" int dfn_isosurface_count(const float* sigma, int nx, int ny, int nz, float iso, void* workspace, size_t workspace_bytes,
                                    unsigned long long* totals, void* stream) {
  using namespace dfn;
  using namespace dfn::iso;
  if (const int rc = check_dims("dfn_isosurface_count", nx, ny, nz)) return rc;
  if (!sigma || !workspace || !totals) return set_error(DFN_ERR_ARG, "dfn_isosurface_count: null pointer");
  const Grid g = make_grid(nx, ny, nz);
  const Layout L = layout(g.n);
  if (workspace_bytes < L.total)
    return set_error(DFN_ERR_ARG, "dfn_isosurface_count: workspace of %zu bytes, dfn_isosurface_workspace_bytes gives %zu", workspace_bytes, L.total);
  char* ws = static_cast<char*>(workspace);
  uint32_t *vpre = reinterpret_cast<uint32_t*>(ws + L.vpre), *fpre = reinterpret_cast<uint32_t*>(ws + L.fpre);
  uint32_t *vsum = reinterpret_cast<uint32_t*>(ws + L.vsum), *fsum = reinterpret_cast<uint32_t*>(ws + L.fsum);
  const uint32_t nb = (g.n + kScan - 1) / kScan;
  hipStream_t s = static_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(count_kernel, dim3(nb), dim3(kScan), 0, s, sigma, g, iso, vpre, fpre, vsum, fsum, reinterpret_cast<uint8_t*>(ws + L.bits));
  hipLaunchKernelGGL(scan_sums_kernel, dim3(1), dim3(kTop), 0, s, vsum, fsum, nb, totals);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return set_error(DFN_ERR_HIP, "dfn_isosurface_count: %s", hipGetErrorString(e));
  return DFN_OK;
}

extern "C" int dfn_isosurface_emit(const float* sigma, const float* xs, const float* ys, const float* zs, int nx, int ny, int nz, float iso,
                                   const void* workspace, size_t workspace_bytes, float* verts, long long V, int* faces, long long F,
                                   void* stream) {
  using namespace dfn;
  using namespace dfn::iso;
  if (const int rc = check_dims("dfn_isosurface_emit", nx, ny, nz)) return rc;
  if (!sigma || !xs || !ys || !zs || !workspace) return set_error(DFN_ERR_ARG, "dfn_isosurface_emit: null pointer");
  const Grid g = make_grid(nx, ny, nz);
  const Layout L = layout(g.n);
  if (workspace_bytes < L.total)
    return set_error(DFN_ERR_ARG, "dfn_isosurface_emit: workspace of %zu bytes, dfn_isosurface_workspace_bytes gives %zu", workspace_bytes, L.total);
  if (V < 0 || F < 0 || V > 7LL * g.n || F > 12LL * g.n)
    return set_error(DFN_ERR_ARG, "dfn_isosurface_emit: V = %lld, F = %lld outside what %u nodes can give", V, F, g.n);
  if ((V > 0 && !verts) || (F > 0 && !faces)) return set_error(DFN_ERR_ARG, "dfn_isosurface_emit: null output for a non-empty result");
  if (V == 0 && F == 0) return DFN_OK;
  const char* ws = static_cast<const char*>(workspace);
  Prefix p;
  p.vpre = reinterpret_cast<const uint32_t*>(ws + L.vpre), p.fpre = reinterpret_cast<const uint32_t*>(ws + L.fpre);
  p.vsum = reinterpret_cast<const uint32_t*>(ws + L.vsum), p.fsum = reinterpret_cast<const uint32_t*>(ws + L.fsum);
  p.bits = reinterpret_cast<const uint8_t*>(ws + L.bits);
  hipLaunchKernelGGL(emit_kernel, dim3((g.n + 255) / 256), dim3(256), 0, static_cast<hipStream_t>(stream), sigma, xs, ys, zs, g, iso, p,
                     verts, (uint32_t)V, faces, (uint32_t)F);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return set_error(DFN_ERR_HIP, "dfn_isosurface_emit: %s", hipGetErrorString(e));
  return DFN_OK;
}
