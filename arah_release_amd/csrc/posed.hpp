// Posed-space queries of the articulated SDF (arah_query_posed, arah_sdf_grid_posed; DESIGN.md section 4, "Posed queries").
//
// A posed point x gets exactly what the eval forward computes for a depth sample at x: nearest SMPL vertex + inverse LBS
// (RT:408-421), Broyden on LBS(x_hat) - (x - trans) (loop C, RFU:267-362), the SDF trunk at the normalised solution (IDR:336-359).
// The production kernels do that work; what lives here is the flat-list driver's own part:
//   k_posed_pick    the chunk's points (a caller list, or lattice points formed on the device), minus the ones the occupancy
//                   bitmap certifies, compacted into a dense work list -- one ballot per 64 points, one atomic per wave;
//   k_posed_norm    normalisation of the solutions and the convergence flag (k_canon_finalize's rule);
//   k_posed_out     the scatter back into the caller's order (and the lattice's value rule);
//   k_posed_box_*   the default lattice box: the bounding box of the bitmap's marked voxels, one voxel of margin, as a cube.
// Work arrays are indexed by the position j in the compacted list, so every kernel of the chain sees a dense list 0 .. count.
// The per-point results of the chain do not depend on which other points share the list (the property the tiered forward rests
// on): a point gives the same bits whether or not the bitmap was passed, and wherever it sits in the caller's list.
#pragma once

constexpr int kPosedChunk = 1 << 19;   // points per internal pass: bounds arah_query_posed_bytes whatever the list's length

// where the points of one pass come from
struct PosedSrc {
    const float* pts;   // caller list [n][3] (world metres), or NULL: the lattice below
    const float* box;   // lattice: DEVICE [4] origin xyz, side (metres)
    int n_side;
    int band;           // lattice: 1 = a point is evaluated only when it shares a cell with a lattice point in a marked voxel
};

// lattice point g = (ix * n + iy) * n + iz at origin + (i / (n - 1)) side
__device__ __forceinline__ V3 posed_lattice_point(const float* box, int n, int ix, int iy, int iz) {
    const float inv = 1.0f / (float)(n - 1), side = box[3];
    return V3{box[0] + ((float)ix * inv) * side, box[1] + ((float)iy * inv) * side, box[2] + ((float)iz * inv) * side};
}

// band rule: some lattice point of the 3x3x3 neighbourhood (the points that share a cell with g) lies in a marked voxel
// (occ_lookup: outside the bitmap's box, and on an invalid bitmap, counts as marked)
__device__ __forceinline__ bool posed_band_hit(const OccInfo& oi, const unsigned* bits, const uint8_t* dist, const float* box, int n,
                                               int ix, int iy, int iz) {
    int d;
    for (int a = max(ix - 1, 0); a <= min(ix + 1, n - 1); ++a)
        for (int b = max(iy - 1, 0); b <= min(iy + 1, n - 1); ++b)
            for (int c = max(iz - 1, 0); c <= min(iz + 1, n - 1); ++c)
                if (occ_lookup(oi, bits, dist, posed_lattice_point(box, n, a, b, c), d)) return true;
    return false;
}

// One pass: points base .. base + m of the source.  Certified points get their final value here (query: state 2 and +fill;
// lattice: +fill, counted in counts[2]); the others are appended to the work list: cpts[j], cidx[j] = the point's index, list[j] = j.
__global__ __launch_bounds__(256) void k_posed_pick(PosedSrc src, const OccInfo* __restrict__ info, const unsigned* __restrict__ bits,
                                                    const uint8_t* __restrict__ dist, long long base, int m, float* __restrict__ cpts,
                                                    int* __restrict__ cidx, int* __restrict__ list, int* __restrict__ cnt,
                                                    float* __restrict__ sdf_out, uint8_t* __restrict__ state_out, int* __restrict__ counts) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    const int lane = threadIdx.x & 63;
    bool keep = false, cert = false;
    V3 p{0.f, 0.f, 0.f};
    const long long g = base + i;
    if (i < m) {
        if (src.pts) {
            p = V3{src.pts[g * 3], src.pts[g * 3 + 1], src.pts[g * 3 + 2]};
            if (info) {
                int d;
                cert = !occ_lookup(*info, bits, dist, p, d);
            }
        } else {
            const int n = src.n_side;
            const int iz = (int)(g % n), iy = (int)((g / n) % n), ix = (int)(g / ((long long)n * n));
            p = posed_lattice_point(src.box, n, ix, iy, iz);
            if (src.band && info) cert = !posed_band_hit(*info, bits, dist, src.box, n, ix, iy, iz);
        }
        keep = !cert;
        if (cert) {
            sdf_out[g] = ARAH_POSED_FILL;
            if (state_out) state_out[g] = 2;
        }
    }
    const unsigned long long mk = __ballot(keep);
    int wbase = 0;
    if (lane == 0 && mk) wbase = atomicAdd(&cnt[0], __popcll(mk));
    wbase = __shfl(wbase, 0);
    if (keep) {
        const int j = wbase + __popcll(mk & ((1ull << lane) - 1ull));
        cpts[(size_t)j * 3] = p.x;
        cpts[(size_t)j * 3 + 1] = p.y;
        cpts[(size_t)j * 3 + 2] = p.z;
        cidx[j] = (int)g;
        list[j] = j;
    }
    if (counts) {
        const unsigned long long mc = __ballot(cert);
        if (lane == 0 && mc) atomicAdd(&counts[2], __popcll(mc));
    }
}

// RT:447-461 on the work list: the normalised solution and converged = |g|_best < thr
__global__ __launch_bounds__(256) void k_posed_norm(FrameDev fr, const int* __restrict__ cnt, const float* __restrict__ xraw,
                                                    const float* __restrict__ err, float* __restrict__ xn, uint8_t* __restrict__ conv) {
    const int n = cnt[0];
    const BodyConst bc = load_bc(fr);
    for (int j = blockIdx.x * blockDim.x + threadIdx.x; j < n; j += gridDim.x * blockDim.x) {
        const V3 q = normalize_pt(bc, V3{xraw[(size_t)j * 3], xraw[(size_t)j * 3 + 1], xraw[(size_t)j * 3 + 2]});
        xn[(size_t)j * 3] = q.x;
        xn[(size_t)j * 3 + 1] = q.y;
        xn[(size_t)j * 3 + 2] = q.z;
        conv[j] = err[j] < kRootThresh ? 1 : 0;
    }
}

struct PosedOut {       // the caller's arrays (any of the optional ones may be NULL)
    float* sdf;         // [P] metres (lattice: the value rule)
    float* x_hat_norm;  // [P][3]
    float* T;           // [P][16]
    float* normal;      // [P][3]
    float* weights;     // [P][24]
    uint8_t* state;     // [P]
    int* counts;        // lattice: [3] evaluated, converged, certified
};

// scatter of the work list into the caller's order.  sdf in metres (IDR:359); normal = normalize(T[:3,:3] grad), the posed normal of
// arah_render_maps, formed the same way.  Lattice (out.state == NULL): converged points take their sdf, the others +fill.
__global__ __launch_bounds__(256) void k_posed_out(FrameDev fr, const int* __restrict__ cnt, const int* __restrict__ cidx,
                                                   const float* __restrict__ sdfn, const uint8_t* __restrict__ conv,
                                                   const float* __restrict__ xn, const float* __restrict__ Tw, const float* __restrict__ grad,
                                                   const float* __restrict__ wts, PosedOut out) {
    const int n = cnt[0];
    const BodyConst bc = load_bc(fr);
    const float scale = sdf_scale(bc);
    for (int j0 = blockIdx.x * blockDim.x; j0 < n; j0 += gridDim.x * blockDim.x) {
        const int j = j0 + threadIdx.x;
        const bool live = j < n;
        const bool ok = live && conv[j];
        if (live) {
            const long long g = cidx[j];
            const float s = sdfn[j] * scale;
            if (!out.state) {
                out.sdf[g] = ok ? s : ARAH_POSED_FILL;
            } else {
                out.sdf[g] = s;
                out.state[g] = ok ? 1 : 0;
                const float* Tq = Tw + (size_t)j * 16;
                if (out.x_hat_norm)
                    for (int c = 0; c < 3; ++c) out.x_hat_norm[g * 3 + c] = xn[(size_t)j * 3 + c];
                if (out.T)
                    for (int c = 0; c < 4; ++c)
                        reinterpret_cast<f32x4*>(out.T + g * 16)[c] = reinterpret_cast<const f32x4*>(Tq)[c];
                if (out.normal) {
                    const float nx = grad[(size_t)j * 3], ny = grad[(size_t)j * 3 + 1], nz = grad[(size_t)j * 3 + 2];
                    const float ax = Tq[0] * nx + Tq[1] * ny + Tq[2] * nz;
                    const float ay = Tq[4] * nx + Tq[5] * ny + Tq[6] * nz;
                    const float az = Tq[8] * nx + Tq[9] * ny + Tq[10] * nz;
                    const float len = fmaxf(sqrtf(ax * ax + ay * ay + az * az), 1e-12f);
                    out.normal[g * 3] = ax / len;
                    out.normal[g * 3 + 1] = ay / len;
                    out.normal[g * 3 + 2] = az / len;
                }
                if (out.weights)
                    for (int c = 0; c < 24; ++c) out.weights[g * 24 + c] = wts[(size_t)j * 24 + c];
            }
        }
        if (out.counts) {
            const int lane = threadIdx.x & 63;
            const unsigned long long me = __ballot(live), mc = __ballot(ok);
            if (lane == 0 && me) atomicAdd(&out.counts[0], __popcll(me));
            if (lane == 0 && mc) atomicAdd(&out.counts[1], __popcll(mc));
        }
    }
}

// ---- default lattice box: voxel-index bounds of the marked voxels ([0..2] min, [3..5] max), then the cube
__global__ void k_posed_box_begin(int* bounds) {
    const int t = threadIdx.x;
    if (t < 6) bounds[t] = t < 3 ? 0x7fffffff : -1;
}

__global__ __launch_bounds__(256) void k_posed_box_reduce(const OccInfo* __restrict__ info, const unsigned* __restrict__ bits, int* bounds) {
    const OccInfo oi = *info;
    int lo[3] = {0x7fffffff, 0x7fffffff, 0x7fffffff}, hi[3] = {-1, -1, -1};
    if (oi.valid) {
        const int words = (oi.n_vox + 31) / 32;
        for (int wi = blockIdx.x * blockDim.x + threadIdx.x; wi < words; wi += gridDim.x * blockDim.x) {
            unsigned w = bits[wi];
            while (w) {
                const int b = wi * 32 + __ffs((int)w) - 1;
                w &= w - 1;
                if (b >= oi.n_vox) break;
                const int v[3] = {b % oi.dims[0], (b / oi.dims[0]) % oi.dims[1], b / (oi.dims[0] * oi.dims[1])};
                for (int a = 0; a < 3; ++a) {
                    lo[a] = min(lo[a], v[a]);
                    hi[a] = max(hi[a], v[a]);
                }
            }
        }
    }
    for (int a = 0; a < 3; ++a)
        for (int o = 32; o > 0; o >>= 1) {
            lo[a] = min(lo[a], __shfl_xor(lo[a], o));
            hi[a] = max(hi[a], __shfl_xor(hi[a], o));
        }
    if ((threadIdx.x & 63) == 0 && hi[0] >= 0)
        for (int a = 0; a < 3; ++a) {
            atomicMin(&bounds[a], lo[a]);
            atomicMax(&bounds[3 + a], hi[a]);
        }
}

// the cube centred on the marked voxels' box grown by one voxel; the whole bitmap box when nothing is marked or the bitmap is invalid
__global__ void k_posed_box_finish(const OccInfo* __restrict__ info, const int* __restrict__ bounds, float* __restrict__ box_out) {
    if (threadIdx.x != 0) return;
    const OccInfo oi = *info;
    float lo[3], hi[3];
    const bool any = oi.valid && bounds[3] >= 0;
    for (int a = 0; a < 3; ++a) {
        lo[a] = oi.origin[a] + (any ? (float)(bounds[a] - 1) : 0.f) * oi.v;
        hi[a] = oi.origin[a] + (any ? (float)(bounds[3 + a] + 2) : (float)oi.dims[a]) * oi.v;
    }
    const float side = fmaxf(fmaxf(hi[0] - lo[0], hi[1] - lo[1]), hi[2] - lo[2]);
    for (int a = 0; a < 3; ++a) box_out[a] = 0.5f * (lo[a] + hi[a]) - 0.5f * side;
    box_out[3] = side;
}
