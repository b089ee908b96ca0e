// meshraster.hpp -- an indexed mesh drawn on the device: pix_to_face, depth and perspective-correct barycentrics per pixel (what
// pytorch3d's MeshRasterizer returns for one face per pixel and no blur), and per-vertex attributes interpolated with them.
//
// The rule is meshing.mesh_rasterize / meshing.interpolate_attributes, and every result equals it bit for bit.  verts (V,3) are
// (u, v, view depth) per vertex, pixel (i, j) has its centre at px = j + 0.5, py = i + 0.5.  All float32 arithmetic is rounded
// operation by operation (contraction off):
//
//   * a face is VALID when its ids lie in [0, V), its three z are finite and > z_near, and area2 = (x1-x0)(y2-y0) - (x2-x0)(y1-y0)
//     is finite and not 0 (cull = 1 also drops area2 < 0, cull = 2 area2 > 0);
//   * its pixels are those whose centres lie in the closed bounding box of its three vertices, clipped to the image: columns
//     max(ceil(xmin - 0.5), 0) .. min(floor(xmax - 0.5), W - 1), rows alike -- whatever the size of that box;
//   * e0 = E(1,2), e1 = E(2,0), e2 = E(0,1) with E(a,b) = (xa-px)(yb-py) - (xb-px)(ya-py); E(a,b) is -E(b,a) bit for bit.  The
//     pixel is covered when all three are >= 0 (area2 > 0) or all <= 0 (area2 < 0) and s = (e0+e1)+e2 != 0;
//   * the fragment's depth is z = 1 / (((e0/z0 + e1/z1) + e2/z2) / s), dropped unless finite and > 0;
//   * the pixel goes to the smallest 64-bit key (bits(z) << 32) | face: the nearest face, the lowest id on an exact tie;
//   * the winner's barycentrics, in float64 from the float32 e_k: b_k = e_k / ((e0+e1)+e2), p_k = b_k / z_k,
//     bary_k = float32(p_k / ((p0+p1)+p2)); background: pix_to_face = depth = bary = -1.
//
// arah_mesh_rasterize, one launch per line:
//
//   k_mr_init      every key = ~0, the two list counters = 0
//   k_mr_scatter   pass A.  One lane per face sets it up and sorts it by the pixels n of its clipped bounding box:
//                    n <= small_area   the lane draws it alone (a marching-cubes triangle of the 256^3 body covers 4 at 512^2)
//                    n <= wave_area    the wave draws it, the large faces of the 64 in turn (mesh_wave_turns of meshcommon.hpp): their
//                                      set-up is broadcast (shuffle) and the 64 lanes stride over the box, at most wave_area / 64 rounds
//                    n <= huge_area    the face id is appended to the MEDIUM list
//                    more              ... to the HUGE list
//   k_mr_lists     the two lists (mesh_list_walk of meshcommon.hpp): an image-covering face is spread over kMrParts workgroups
//   k_mr_resolve   pass B.  One thread per pixel decodes the winner, recomputes its e_k in the same arithmetic and writes the three
//                  outputs
//
// The lists and their counters live in the OUTPUTS, which pass B overwrites afterwards: the medium list in pix_to_face, the huge
// list in depth (H W ids each), the counters in bary[0] and bary[1]: no scratch.  A face that finds its list full (more than H W
// of a kind) is drawn by its wave instead.  Why lists and not the wave alone: a coarse mesh has few faces, so few waves, and a
// wave that draws its 64 large faces one after the other leaves the device idle (measured).
// The only atomic that decides a result is the 64-bit integer atomicMin of pass A: a minimum does not depend on the order of
// arrival, so neither does the image.  (The lists' order does depend on it and is never seen.)  No thread waits for another: no
// spin-wait, no grid-wide barrier, nothing persistent; every loop ends by an argument of its own, stated at the loop.
#pragma once

constexpr int kMrMaxGrid = 1 << 14;      // the walkers' cap (meshcontains.hpp's too), a quarter of kImeshMaxGrid
// the three thresholds as measured on the 256^3 body and its simplified meshes at 512^2 and 1024^2 (profiles/mesh_render_bench.txt)
constexpr int kMrSmallArea = 16;         // pixels of a clipped bounding box one lane still walks alone
constexpr int kMrWaveArea = 64;          // ... the face's wave still walks: one round of its 64 lanes
constexpr int kMrHugeArea = 4096;        // ... one workgroup still walks: 16 pixels a thread
constexpr int kMrParts = 64;             // parts, and workgroups, of a face above that
constexpr int kMrListGrid = 2048;        // workgroups of k_mr_lists
constexpr unsigned long long kMrEmpty = ~0ull;

struct MrFace {
    float x0, y0, z0, x1, y1, z1, x2, y2, z2;
    int j0, i0, w, n;   // first column and row of the clipped box, its width and its pixels (n <= H W < 2^31)
    int pos;            // area2 > 0
};

// Face f set up: false when it is not valid or its clipped box is empty
__device__ __forceinline__ bool mr_setup(const float* __restrict__ verts, int n_verts, const int* __restrict__ faces, long long f, int H,
                                         int W, float z_near, int cull, MrFace& t) {
#pragma clang fp contract(off)
    int id[3];
    if (!cc_face_ok(faces, f, n_verts, id)) return false;
    const float* a = verts + 3 * (size_t)id[0];
    const float* b = verts + 3 * (size_t)id[1];
    const float* c = verts + 3 * (size_t)id[2];
    t.x0 = a[0], t.y0 = a[1], t.z0 = a[2];
    t.x1 = b[0], t.y1 = b[1], t.z1 = b[2];
    t.x2 = c[0], t.y2 = c[1], t.z2 = c[2];
    if (!(t.z0 > z_near && t.z1 > z_near && t.z2 > z_near)) return false;
    if (!(isfinite(t.z0) && isfinite(t.z1) && isfinite(t.z2))) return false;
    const float area2 = (t.x1 - t.x0) * (t.y2 - t.y0) - (t.x2 - t.x0) * (t.y1 - t.y0);
    if (!isfinite(area2) || area2 == 0.0f) return false;
    if ((cull == 1 && area2 < 0.0f) || (cull == 2 && area2 > 0.0f)) return false;
    t.pos = area2 > 0.0f;
    // a finite area2 has finite x and y.  The box in float, held to [-1, the largest float below 2^31] before it becomes an int
    const float lim = 2147483520.0f;
    const float xmin = fminf(t.x0, fminf(t.x1, t.x2)), xmax = fmaxf(t.x0, fmaxf(t.x1, t.x2));
    const float ymin = fminf(t.y0, fminf(t.y1, t.y2)), ymax = fmaxf(t.y0, fmaxf(t.y1, t.y2));
    const int j0 = max((int)fminf(fmaxf(ceilf(xmin - 0.5f), -1.0f), lim), 0);
    const int j1 = min((int)fminf(fmaxf(floorf(xmax - 0.5f), -1.0f), lim), W - 1);
    const int i0 = max((int)fminf(fmaxf(ceilf(ymin - 0.5f), -1.0f), lim), 0);
    const int i1 = min((int)fminf(fmaxf(floorf(ymax - 0.5f), -1.0f), lim), H - 1);
    if (j1 < j0 || i1 < i0) return false;
    t.j0 = j0, t.i0 = i0, t.w = j1 - j0 + 1;
    t.n = t.w * (i1 - i0 + 1);   // <= H W <= INT32_MAX
    return true;
}

__device__ __forceinline__ void mr_edges(const MrFace& t, int i, int j, float& e0, float& e1, float& e2) {
#pragma clang fp contract(off)
    const float px = (float)j + 0.5f, py = (float)i + 0.5f;
    const float dx0 = t.x0 - px, dx1 = t.x1 - px, dx2 = t.x2 - px;
    const float dy0 = t.y0 - py, dy1 = t.y1 - py, dy2 = t.y2 - py;
    e0 = dx1 * dy2 - dx2 * dy1;
    e1 = dx2 * dy0 - dx0 * dy2;
    e2 = dx0 * dy1 - dx1 * dy0;
}

// Pixels first, first + stride, ... of the face's clipped box, in row-major order of the box: every covered one offers its key.
// i <= i1 < H and j <= j1 < W by the set-up, so the key written lies inside the H W keys
__device__ __forceinline__ void mr_draw(const MrFace& t, unsigned face, unsigned first, unsigned last, unsigned stride, int W,
                                        unsigned long long* __restrict__ keys) {
#pragma clang fp contract(off)
    // terminates: last - p strictly decreases (stride >= 1); p + stride < 2^31 + 2^24 does not wrap
    for (unsigned p = first; p < last; p += stride) {
        const unsigned row = p / (unsigned)t.w;
        const int i = t.i0 + (int)row, j = t.j0 + (int)(p - row * (unsigned)t.w);
        float e0, e1, e2;
        mr_edges(t, i, j, e0, e1, e2);
        const bool in = t.pos ? (e0 >= 0.0f && e1 >= 0.0f && e2 >= 0.0f) : (e0 <= 0.0f && e1 <= 0.0f && e2 <= 0.0f);
        const float s = (e0 + e1) + e2;
        if (!in || s == 0.0f) continue;
        const float q = ((e0 / t.z0 + e1 / t.z1) + e2 / t.z2) / s;
        const float z = 1.0f / q;
        if (!(isfinite(z) && z > 0.0f)) continue;
        atomicMin(&keys[(size_t)i * W + j], ((unsigned long long)__float_as_uint(z) << 32) | face);
    }
}

__global__ __launch_bounds__(kImeshThreads) void k_mr_init(unsigned long long* __restrict__ keys, long long n_pix, unsigned* __restrict__ counters) {
    const long long step = (long long)gridDim.x * blockDim.x;
    // terminates: n_pix - p strictly decreases (step >= 1) and the loop ends when it reaches 0
    for (long long p = (long long)blockIdx.x * blockDim.x + threadIdx.x; p < n_pix; p += step) keys[p] = kMrEmpty;
    if (blockIdx.x == 0 && threadIdx.x < 2) counters[threadIdx.x] = 0u;
}

__global__ __launch_bounds__(kImeshThreads) void k_mr_scatter(const float* __restrict__ verts, int n_verts, const int* __restrict__ faces,
                                                              int n_faces, int H, int W, float z_near, int cull, int small_area,
                                                              int wave_area, int huge_area, unsigned long long* __restrict__ keys,
                                                              int* __restrict__ med_list, int* __restrict__ huge_list, unsigned cap,
                                                              unsigned* counters) {
    const long long step = (long long)gridDim.x * blockDim.x, end = ((long long)n_faces + 63) & ~63ll;
    const unsigned lane = threadIdx.x & 63;
    // terminates: end - f strictly decreases (step >= 1) and the loop ends when it reaches 0.  The face count is rounded up to
    // whole waves and step is a multiple of 64, so all 64 lanes of a wave reach the ballot together; lanes beyond the end carry
    // no face
    for (long long f = (long long)blockIdx.x * blockDim.x + threadIdx.x; f < end; f += step) {
        MrFace t;
        t.x0 = t.y0 = t.z0 = t.x1 = t.y1 = t.z1 = t.x2 = t.y2 = t.z2 = 0.0f;
        t.j0 = t.i0 = t.w = t.n = t.pos = 0;
        const bool ok = f < n_faces && mr_setup(verts, n_verts, faces, f, H, W, z_near, cull, t);
        bool large = false;
        if (ok) {
            if (t.n <= small_area) {
                mr_draw(t, (unsigned)f, 0u, (unsigned)t.n, 1u, W, keys);
            } else if (t.n <= wave_area) {
                large = true;
            } else {
                const int huge = t.n > huge_area;
                const unsigned slot = atomicAdd(&counters[huge], 1u);   // at most n_faces < 2^31 increments: no wrap
                if (slot < cap) (huge ? huge_list : med_list)[slot] = (int)f;
                else large = true;                                       // the list is full: the wave draws it
            }
        }
        mesh_wave_turns(large, [&](int src) {
            MrFace b;
            b.x0 = __shfl(t.x0, src), b.y0 = __shfl(t.y0, src), b.z0 = __shfl(t.z0, src);
            b.x1 = __shfl(t.x1, src), b.y1 = __shfl(t.y1, src), b.z1 = __shfl(t.z1, src);
            b.x2 = __shfl(t.x2, src), b.y2 = __shfl(t.y2, src), b.z2 = __shfl(t.z2, src);
            b.j0 = __shfl(t.j0, src), b.i0 = __shfl(t.i0, src), b.w = __shfl(t.w, src), b.n = __shfl(t.n, src);
            b.pos = __shfl(t.pos, src);
            // the lanes of one wave hold 64 consecutive faces: the source lane's is f - lane + src
            mr_draw(b, (unsigned)(f - lane + src), lane, (unsigned)b.n, 64u, W, keys);
        });
    }
}

__global__ __launch_bounds__(kImeshThreads) void k_mr_lists(const float* __restrict__ verts, int n_verts, const int* __restrict__ faces,
                                                            int n_faces, int H, int W, float z_near, int cull,
                                                            unsigned long long* __restrict__ keys, const int* __restrict__ med_list,
                                                            const int* __restrict__ huge_list, unsigned cap,
                                                            const unsigned* __restrict__ counters) {
    mesh_list_walk<kMrParts, kImeshThreads, MrFace>(
        med_list, min(counters[0], cap), huge_list, min(counters[1], cap),
        [&](int f, MrFace& t) {   // the set-up is run again: a list holds ids only
            return (unsigned)f < (unsigned)n_faces && mr_setup(verts, n_verts, faces, f, H, W, z_near, cull, t) ? (unsigned)t.n : 0u;
        },
        [&](int f, const MrFace& t, unsigned first, unsigned last, unsigned stride) { mr_draw(t, (unsigned)f, first, last, stride, W, keys); });
}

__global__ __launch_bounds__(kImeshThreads) void k_mr_resolve(const float* __restrict__ verts, int n_verts, const int* __restrict__ faces,
                                                              int n_faces, int H, int W, const unsigned long long* __restrict__ keys,
                                                              int* __restrict__ pix_to_face, float* __restrict__ depth,
                                                              float* __restrict__ bary) {
#pragma clang fp contract(off)
    const long long step = (long long)gridDim.x * blockDim.x, n_pix = (long long)H * W;
    // terminates: n_pix - p strictly decreases (step >= 1) and the loop ends when it reaches 0
    for (long long p = (long long)blockIdx.x * blockDim.x + threadIdx.x; p < n_pix; p += step) {
        const unsigned long long key = keys[p];
        int face = -1;
        float z = -1.0f, b[3] = {-1.0f, -1.0f, -1.0f};
        const int f = (int)(unsigned)(key & 0xffffffffull);
        int id[3];
        if (key != kMrEmpty && (unsigned)f < (unsigned)n_faces && cc_face_ok(faces, f, n_verts, id)) {
            MrFace t;
            const float* v0 = verts + 3 * (size_t)id[0];
            const float* v1 = verts + 3 * (size_t)id[1];
            const float* v2 = verts + 3 * (size_t)id[2];
            t.x0 = v0[0], t.y0 = v0[1], t.z0 = v0[2];
            t.x1 = v1[0], t.y1 = v1[1], t.z1 = v1[2];
            t.x2 = v2[0], t.y2 = v2[1], t.z2 = v2[2];
            float e0, e1, e2;
            const unsigned row = (unsigned)p / (unsigned)W;   // p < H W < 2^31
            mr_edges(t, (int)row, (int)((unsigned)p - row * (unsigned)W), e0, e1, e2);
            const double E0 = (double)e0, E1 = (double)e1, E2 = (double)e2;
            const double S = (E0 + E1) + E2;
            const double p0 = (E0 / S) / (double)t.z0, p1 = (E1 / S) / (double)t.z1, p2 = (E2 / S) / (double)t.z2;
            const double P = (p0 + p1) + p2;
            face = f;
            z = __uint_as_float((unsigned)(key >> 32));
            b[0] = (float)(p0 / P), b[1] = (float)(p1 / P), b[2] = (float)(p2 / P);
        }
        pix_to_face[p] = face;
        depth[p] = z;
        bary[3 * p + 0] = b[0];
        bary[3 * p + 1] = b[1];
        bary[3 * p + 2] = b[2];
    }
}

// ---- attributes: three rows of attr (V,C) gathered per pixel and mixed with bary, one thread per (pixel, channel) ---------------------
__global__ __launch_bounds__(kImeshThreads) void k_mr_interpolate(const int* __restrict__ pix_to_face, const float* __restrict__ bary,
                                                                  long long n_pix, const int* __restrict__ faces, int n_faces,
                                                                  const float* __restrict__ attr, int n_verts, int C, float background,
                                                                  float* __restrict__ out) {
#pragma clang fp contract(off)
    const long long step = (long long)gridDim.x * blockDim.x, n = n_pix * C;
    // terminates: n - q strictly decreases (step >= 1) and the loop ends when it reaches 0
    for (long long q = (long long)blockIdx.x * blockDim.x + threadIdx.x; q < n; q += step) {
        const long long p = q / C;
        const int c = (int)(q - p * C);
        const int f = pix_to_face[p];
        float v = background;
        int id[3];
        // pix_to_face is the caller's: a pixel that names no face of THIS mesh, or a face with an id out of range, is background
        if ((unsigned)f < (unsigned)n_faces && cc_face_ok(faces, f, n_verts, id)) {
            const double b0 = (double)bary[3 * p + 0], b1 = (double)bary[3 * p + 1], b2 = (double)bary[3 * p + 2];
            const double a0 = (double)attr[(size_t)id[0] * C + c], a1 = (double)attr[(size_t)id[1] * C + c];
            const double a2 = (double)attr[(size_t)id[2] * C + c];
            v = (float)((b0 * a0 + b1 * a1) + b2 * a2);
        }
        out[q] = v;
    }
}
