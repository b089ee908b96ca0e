// meshray.hpp -- rays against LARGE triangle soups: the first hit (t, face, barycentrics) or any hit, on the uniform grid of
// meshdist.hpp (the index is read, never changed).  DESIGN.md "Casting rays against meshes on the device".
//
//   k_rc_cast<ANY>   one thread per ray: the big list, then the grid's slabs of cells along the ray's major axis
//
// The rule is meshing.mesh_raycast (Woop, Benthin, Wald: "Watertight Ray/Triangle Intersection", JCGT 2013) in float64 on the
// float32 inputs, every operation rounded on its own (contraction off): rc_test() below is that rule for one ray and one face,
// line by line -- including its last condition, that the accepted point of the face lies ON the ray within 2^-26 of the
// coordinates' magnitude, which is what makes the walk's argument hold for every input.  The answer of a ray is the lexicographic minimum of (t, face) over the accepted faces, so the order in which
// the references are met cannot change it; a face met twice (it is referenced from several cells) gives the same candidate twice.
//
// Exactness: the kernel tests a SUBSET of the faces with the arithmetic of the specification, so it equals the specification
// when the specification's winner is in the subset.  The argument is stated at the walk.  Included by arah_hip.hip after
// meshdist.hpp.
#pragma once

namespace {

constexpr int kRcThreads = 64;   // rays per workgroup: one wave (64 / 128 / 256 measured)

struct RcRay {
    double o[3], d[3];
    double ox, oy, oz;   // o[kx], o[ky], o[kz]
    double dx, dy, dz;   // d[kx], d[ky], d[kz]
    double omax;         // the largest |o[c]|
    double Sx, Sy, Sz;
    int kx, ky, kz;
};

// md_cell_of with the axis' figures picked beforehand
__device__ __forceinline__ int rc_cell_of(double lo, double inv_h, int top, double x) {
    const double u = floor((x - lo) * inv_h);
    return !(u > 0.0) ? 0 : (u >= (double)top ? top : (int)u);   // a NaN goes to cell 0: never out of the grid
}

// a[k] without indexing registers by a variable
__device__ __forceinline__ double rc_pick(const double* a, int k) { return k == 0 ? a[0] : (k == 1 ? a[1] : a[2]); }
__device__ __forceinline__ int rc_pick(const int* a, int k) { return k == 0 ? a[0] : (k == 1 ? a[1] : a[2]); }

struct RcHit {
    double t, u, v, w;   // t and the barycentrics U / det, V / det, W / det
    int face;
};

// one ray, one face: true and (t, barycentrics) when the face is accepted within [t_min, t_max]
__device__ __forceinline__ bool rc_test(const RcRay& r, const float* __restrict__ v, double t_min, double t_max, int cull, double& t,
                                        double& bu, double& bv, double& bw) {
#pragma clang fp contract(off)
    const double Az = (double)v[r.kz] - r.oz, Bz = (double)v[3 + r.kz] - r.oz, Cz = (double)v[6 + r.kz] - r.oz;
    const double Ax0 = (double)v[r.kx] - r.ox, Ay0 = (double)v[r.ky] - r.oy;
    const double Bx0 = (double)v[3 + r.kx] - r.ox, By0 = (double)v[3 + r.ky] - r.oy;
    const double Cx0 = (double)v[6 + r.kx] - r.ox, Cy0 = (double)v[6 + r.ky] - r.oy;
    const double Ax = Ax0 - r.Sx * Az, Ay = Ay0 - r.Sy * Az;
    const double Bx = Bx0 - r.Sx * Bz, By = By0 - r.Sy * Bz;
    const double Cx = Cx0 - r.Sx * Cz, Cy = Cy0 - r.Sy * Cz;
    const double U = Cx * By - Cy * Bx;
    const double V = Ax * Cy - Ay * Cx;
    const double W = Bx * Ay - By * Ax;
    if ((U < 0.0 || V < 0.0 || W < 0.0) && (U > 0.0 || V > 0.0 || W > 0.0)) return false;
    const double det = (U + V) + W;
    if (det == 0.0) return false;
    if ((cull == 1 && det < 0.0) || (cull == 2 && det > 0.0)) return false;
    t = ((U * (r.Sz * Az) + V * (r.Sz * Bz)) + W * (r.Sz * Cz)) / det;
    // a NaN fails every comparison; the index's status is 0 here, so every vertex is finite
    if (!(fabs(t) <= 1.7976931348623157e308 && t >= t_min && t <= t_max)) return false;
    // ON THE RAY: the point bary . corners, relative to the origin, against t d, per axis, within 2^-26 of the largest
    // magnitude among the origin's and the corners' coordinates.  A det that is rounding noise (a ray in the face's plane)
    // passes everything above with a point far beside the ray; it fails here.
    bu = U / det;
    bv = V / det;
    bw = W / det;
    double m = r.omax;
#pragma unroll
    for (int k = 0; k < 9; ++k) m = fmax(m, fabs((double)v[k]));
    const double tol = m * 0x1p-26;
    const double rx = ((bu * Ax0 + bv * Bx0) + bw * Cx0) - t * r.dx;
    const double ry = ((bu * Ay0 + bv * By0) + bw * Cy0) - t * r.dy;
    const double rz = ((bu * Az + bv * Bz) + bw * Cz) - t * r.dz;
    return fabs(rx) <= tol && fabs(ry) <= tol && fabs(rz) <= tol;
}

// origins, dirs [R][3] float32 -> ANY false: t [R] f64, face [R] i32, bary [R][3] f64;  true: hit [R] u8.  tested [R] i32 or null.
template <bool ANY>
__global__ __launch_bounds__(256) void k_rc_cast(const float* __restrict__ tris, const MdHeader* __restrict__ hdr, const int* __restrict__ cell_base,
                          const uint8_t* __restrict__ dt, const int* __restrict__ refs, const int* __restrict__ big,
                          const float* __restrict__ origins, const float* __restrict__ dirs, int n_rays, double t_min, double t_max,
                          int cull, double* __restrict__ t_out, int* __restrict__ face_out, double* __restrict__ bary_out,
                          uint8_t* __restrict__ hit_out, int* __restrict__ tested_out) {
#pragma clang fp contract(off)
    const int i = blockIdx.x * blockDim.x + threadIdx.x;   // n_rays <= 2^31 - 1 - 256 (arah_mesh_raycast): no overflow
    if (i >= n_rays) return;
    const MdHeader H = *hdr;
    const double inf = __longlong_as_double(0x7ff0000000000000ll);
    RcRay r;
    bool valid = H.status == 0, nonzero = false;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        r.o[c] = (double)origins[(size_t)i * 3 + c];
        r.d[c] = (double)dirs[(size_t)i * 3 + c];
        valid = valid && fabs(r.o[c]) <= kMdFltMax && fabs(r.d[c]) <= kMdFltMax;
        nonzero = nonzero || r.d[c] != 0.0;
    }
    valid = valid && nonzero;
    RcHit best = {inf, 0.0, 0.0, 0.0, -1};
    int tested = 0;
    bool found = false;   // ANY: a face was accepted
    if (valid) {
        const double ax = fabs(r.d[0]), ay = fabs(r.d[1]), az = fabs(r.d[2]);
        r.kz = (ax >= ay && ax >= az) ? 0 : (ay >= az ? 1 : 2);
        r.kx = (r.kz + 1) % 3;
        r.ky = (r.kx + 1) % 3;
        const double dkz = rc_pick(r.d, r.kz);
        if (dkz < 0.0) {
            const int s = r.kx;
            r.kx = r.ky;
            r.ky = s;
        }
        r.ox = rc_pick(r.o, r.kx);
        r.oy = rc_pick(r.o, r.ky);
        r.oz = rc_pick(r.o, r.kz);
        r.Sx = rc_pick(r.d, r.kx) / dkz;
        r.Sy = rc_pick(r.d, r.ky) / dkz;
        r.Sz = 1.0 / dkz;
        r.dx = rc_pick(r.d, r.kx);
        r.dy = rc_pick(r.d, r.ky);
        r.dz = dkz;
        r.omax = fmax(fabs(r.o[0]), fmax(fabs(r.o[1]), fabs(r.o[2])));
        auto test = [&](int f) {
            double t, bu, bv, bw;
            ++tested;
            if (!rc_test(r, tris + (size_t)f * 9, t_min, t_max, cull, t, bu, bv, bw)) return;
            found = true;
            if (t < best.t || (t == best.t && f < best.face)) best = RcHit{t, bu, bv, bw, f};
        };
        // the big list: n_big <= n_faces trips
        for (int k = 0; k < H.n_big && !(ANY && found); ++k) test(big[k]);

        // ---- the walk -------------------------------------------------------------------------------------------------------
        // What has to be visited.  An accepted face has U, V, W of one sign, so its barycentrics lie in [0, 1] and
        // q = bary . (a, b, c) is a point of the triangle (up to a few 2^-52 of its coordinates); and BY THE RULE'S LAST
        // CONDITION q lies within 2^-26 m of the ray's point o + t d along every axis, m the largest magnitude among the origin
        // and the face's corners -- the rule does not leave this to the conditioning of det.  `slack` is 2^-26 M with M the
        // largest magnitude among the origin and the BOX's corners, so M >= m, plus 2^-20 cells for the rounding of md_cell_of
        // (within 2^-40 of a cell); every bound below is widened by 2 slack, the second for the bounds' own rounding and that
        // of q and o + t d (a few 2^-52 M).  q lies in the triangle's box, the triangle is referenced from EVERY cell of
        // [md_cell_of(min), md_cell_of(max)] per axis (k_md_bin), and md_cell_of is monotone: so the face is met when the walk
        // visits, for every slab cz of cells along kz, every cell (x, y, cz) with md_cell_of(p_x - 2 slack) <= x <=
        // md_cell_of(p_x + 2 slack) (y alike) for the ray's points p whose kz coordinate lies within 2 slack of the slab -- the
        // two ends of that piece of the ray bound p_x and p_y, which are linear in t.
        double te = t_min, tx = t_max;   // the ray inside the box widened by 2 slack
        double slack = 0.0;
        bool inside = H.n_refs > 0 && !(ANY && found);
        if (inside) {
            double M = 0.0;
#pragma unroll
            for (int a = 0; a < 3; ++a) M = fmax(M, fmax(fabs(r.o[a]), fmax(fabs(H.lo[a]), fabs(H.hi[a]))));
            slack = H.h * 0x1p-20 + M * 0x1p-26;
#pragma unroll
            for (int a = 0; a < 3; ++a) {
                const double l = H.lo[a] - 2.0 * slack, u = H.hi[a] + 2.0 * slack;
                if (r.d[a] == 0.0) {
                    inside = inside && r.o[a] >= l && r.o[a] <= u;
                } else {
                    const double inv = 1.0 / r.d[a];
                    const double t0 = (l - r.o[a]) * inv, t1 = (u - r.o[a]) * inv;
                    te = fmax(te, fmin(t0, t1));
                    tx = fmin(tx, fmax(t0, t1));
                }
            }
            inside = inside && te <= tx;   // d[kz] != 0: te and tx are finite or the interval is empty
        }
        if (inside) {
            const int kz = r.kz, ka = (kz + 1) % 3, kb = (kz + 2) % 3;
            const int strides[3] = {1, H.n[0], H.n[0] * H.n[1]};
            const int sz = rc_pick(strides, kz), sa = rc_pick(strides, ka), sb = rc_pick(strides, kb);
            const double oz = r.oz, dz = rc_pick(r.d, kz), inv_dz = r.Sz;
            const double oa = rc_pick(r.o, ka), da = rc_pick(r.d, ka), ob = rc_pick(r.o, kb), db = rc_pick(r.d, kb);
            const double lo_z = rc_pick(H.lo, kz), lo_a = rc_pick(H.lo, ka), lo_b = rc_pick(H.lo, kb);
            const int top = rc_pick(H.n, kz) - 1, top_a = rc_pick(H.n, ka) - 1, top_b = rc_pick(H.n, kb) - 1;
            const bool up = dz > 0.0, can_skip = 8.0 * slack <= H.h;
            const int step = up ? 1 : -1;
            const double za = oz + te * dz, zb = oz + tx * dz;
            int cz = rc_cell_of(lo_z, H.inv_h, top, up ? za - 2.0 * slack : za + 2.0 * slack);
            const int cz_end = rc_cell_of(lo_z, H.inv_h, top, up ? zb + 2.0 * slack : zb - 2.0 * slack);
            // Ends: cz moves towards cz_end by at least one cell per trip, at most n[kz] <= 1024 trips.  It ends early when the
            // slab's entry parameter ta -- a lower bound, by the 2 slack, on the t of every hit in this slab and in those behind
            // it -- is STRICTLY greater than the best t: a tie in t is still examined.
            while (up ? cz <= cz_end : cz >= cz_end) {
                // the piece [ta, tb] of the ray in the slab widened by 2 slack; the first and the last cell of an axis are
                // clamped (md_cell_of), so their slabs reach to the ends of the ray
                const double z_lo = lo_z + (double)cz * H.h - 2.0 * slack, z_hi = lo_z + (double)(cz + 1) * H.h + 2.0 * slack;
                const bool first_cell = up ? cz == 0 : cz == top, last_cell = up ? cz == top : cz == 0;
                double ta = first_cell ? te : fmax(te, ((up ? z_lo : z_hi) - oz) * inv_dz);
                double tb = last_cell ? tx : fmin(tx, ((up ? z_hi : z_lo) - oz) * inv_dz);
                if (ta > best.t) break;
                if (!ANY) tb = fmin(tb, best.t);
                int kmin = 255;
                if (ta <= tb) {
                    const double a0 = oa + ta * da, a1 = oa + tb * da;
                    const double b0 = ob + ta * db, b1 = ob + tb * db;
                    const int xa = rc_cell_of(lo_a, H.inv_h, top_a, fmin(a0, a1) - 2.0 * slack);
                    const int xb = rc_cell_of(lo_a, H.inv_h, top_a, fmax(a0, a1) + 2.0 * slack);
                    const int ya = rc_cell_of(lo_b, H.inv_h, top_b, fmin(b0, b1) - 2.0 * slack);
                    const int yb = rc_cell_of(lo_b, H.inv_h, top_b, fmax(b0, b1) + 2.0 * slack);
                    // |d[ka]|, |d[kb]| <= |d[kz]|: the piece moves by at most h + 4 slack along ka and kb, a handful of cells
                    for (int y = ya; y <= yb && !(ANY && found); ++y)
                        for (int x = xa; x <= xb && !(ANY && found); ++x) {
                            const int cell = cz * sz + x * sa + y * sb;   // < n_cells
                            const int k = (int)dt[cell];
                            kmin = min(kmin, k);
                            if (k != 0) continue;
                            const int e0 = cell_base[cell], e1 = cell_base[cell + 1];   // e1 <= n_refs
                            for (int e = e0; e < e1; ++e) test(refs[e]);
                        }
                    if (ANY && found) break;
                } else {
                    kmin = 0;   // no piece here (rounding at the box's faces): nothing to test, nothing learnt
                }
                // Empty space.  kmin is the smallest Chebyshev distance, in cells, from a cell just visited to an occupied one.
                // Between the end of this slab and the end of slab cz + j the ray moves j h along kz, so at most j h along ka
                // and kb: the cells visited in slab cz + j lie within j + 2 cells (one for the floor, one for the slack) of
                // those visited here, and are empty when j + 2 < kmin.  Slabs cz + 1 .. cz + kmin - 3 are skipped -- unless the slack
                // is no small part of a cell (a mesh or an origin very far from 0), where "one for the slack" does not hold.
                cz += step * (kmin > 3 && can_skip ? kmin - 2 : 1);
            }
        }
    }
    if (ANY) {
        hit_out[i] = found ? 1 : 0;
    } else {
        t_out[i] = best.t;
        face_out[i] = best.face;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const double n = c == 0 ? best.u : c == 1 ? best.v : best.w;
            bary_out[(size_t)i * 3 + c] = best.face >= 0 ? n : 0.0;
        }
    }
    if (tested_out) tested_out[i] = tested;
}

}  // namespace
