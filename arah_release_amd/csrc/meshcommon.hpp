// meshcommon.hpp -- what the mesh headers share.  The indexed-mesh side (mcubes.hpp, meshcc.hpp, meshsimp.hpp, meshadj.hpp,
// meshquadric.hpp, meshcollapse.hpp, meshsubdiv.hpp, meshorient.hpp, meshraster.hpp, and meshintersect.hpp on the query side's grid): the launch constants, the workgroup prefix, the ordered compaction walk, the
// one-workgroup scan, the padding of the rows between a count and a capacity, and cc_add_one.  The box walkers of both sides
// (meshraster.hpp, meshcontains.hpp, meshsdf.hpp): the wave's turns and the walk of the two lists, at the end of this file.  The
// one-workgroup box reduction of the query side (meshquery.hpp, meshcontains.hpp, meshwinding.hpp).  DESIGN.md ("Indexed meshes:
// the shared walk and the scratch carver") tells the same once, with the host side.  The query side's prefix sums stay out: they
// include a float64 one whose summation order is part of their specification, and integer scans of three widths whose access
// patterns were measured where they are.  The adjacency as a kernel argument (MeshAdj) is meshadj.hpp's, and what the edge
// kernels do with it -- owner fill, entry walk, bisection, merge, float64 helpers -- meshedge.hpp's: they need the adjacency's layout.
//
// COUNT / SCAN / FILL.  Every variable-length result of the indexed-mesh headers is numbered the same way, without atomics, so
// that it is deterministic and keeps the order of its elements:
//
//   count   a walk over the elements; every workgroup writes the number of marked elements of its part -> blk_count[block]
//   scan    k_mc_scan: blk_base = the exclusive scan of blk_count, the total
//   fill    the same walk again; a marked element takes the id blk_base[block] + the marks in front of it inside the part
//
// The part of a workgroup is a lattice row in mcubes.hpp (k_mcubes, k_mc_verts: their own row walks over mesh_prefix) and a chunk
// of kImeshChunk consecutive elements everywhere else (mesh_compact: k_cc_compact, k_ms_compact, k_mo_compact; meshsubdiv.hpp's
// sb_walk is the same chunk walk over mesh_prefix with a weight per element instead of a 0/1 mark).
#pragma once

// "Imesh" = indexed mesh: kMeshThreads = 64 and kMeshChunk = 128 are meshquery.hpp's, the query side's, in the same namespace.
constexpr int kImeshThreads = 256;        // threads of a workgroup of every indexed-mesh kernel
constexpr int kImeshChunk = 1024;          // elements per workgroup of mesh_compact: 4 passes of kImeshThreads
constexpr int kImeshMaxGrid = 1 << 16;     // workgroups of the element-wise walks (they stride over what is left)

// The exclusive prefix of cnt over the workgroup in thread order (the sum of cnt over the threads below this one); total = the
// sum over all kImeshThreads threads.  wsum is the caller's __shared__ int[kImeshThreads / 64].
// CONTRACT: every thread of the workgroup calls it, from workgroup-uniform control flow, once per pass -- it holds two barriers,
// the first before wsum is read, the second before the next pass may write it again.
__device__ __forceinline__ int mesh_prefix(int cnt, int* wsum, int& total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int inc = cnt;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int v = __shfl_up(inc, o);
        if (lane >= o) inc += v;
    }
    if (lane == 63) wsum[wave] = inc;
    __syncthreads();
    int before = 0;
    total = 0;
#pragma unroll
    for (int w = 0; w < kImeshThreads / 64; ++w) {
        if (w < wave) before += wsum[w];
        total += wsum[w];
    }
    __syncthreads();
    return before + inc - cnt;
}

// The count (FILL = false) or fill (FILL = true) walk of a workgroup over its chunk of the n elements, a 0/1 mark per element:
//   mark(i, state) -> bool   called for i < n only; may fill `state`, a State{} of the caller's (a few scalars: registers)
//   emit(i, ok, mark, id, state)   FILL only, called by EVERY thread: ok = i < n, id = the element's id if it is marked
// Ids ascend with the elements, so the order is preserved.  Launch kImeshThreads threads and ceil(n / kImeshChunk) workgroups;
// n is workgroup-uniform, so every thread reaches mesh_prefix in every pass.  `done` cannot overflow: it is at most kImeshChunk.
struct MeshNoState {};

template <bool FILL, class State, class Mark, class Emit>
__device__ __forceinline__ void mesh_compact(long long n, int* __restrict__ blk_count, const int* __restrict__ blk_base, Mark mark,
                                             Emit emit) {
    __shared__ int wsum[kImeshThreads / 64];
    const long long first = (long long)blockIdx.x * kImeshChunk;
    int done = 0;   // marks of this chunk in front of the current pass
#pragma unroll 1
    for (int z0 = 0; z0 < kImeshChunk; z0 += kImeshThreads) {   // terminates: kImeshChunk - z0 strictly decreases to 0
        const long long i = first + z0 + threadIdx.x;
        const bool ok = i < n;
        State state{};
        const bool marked = ok && mark(i, state);
        int total;
        const int before = mesh_prefix(marked ? 1 : 0, wsum, total);
        if constexpr (FILL) emit(i, ok, marked, blk_base[blockIdx.x] + done + before, state);
        done += total;
    }
    if (!FILL && threadIdx.x == 0) blk_count[blockIdx.x] = done;
}

// exclusive scan of n counts by one workgroup: base[i] = sum of count[0 .. i), *total = the sum
__global__ __launch_bounds__(1024) void k_mc_scan(const int* __restrict__ count, int n, int* __restrict__ base, int* total) {
    __shared__ int part[1024];
    const int tid = threadIdx.x;
    const int per = (n + 1023) / 1024;
    const int lo = min(tid * per, n), hi = min(lo + per, n);
    int s = 0;
    for (int i = lo; i < hi; ++i) s += count[i];
    part[tid] = s;
    __syncthreads();
    for (int o = 1; o < 1024; o <<= 1) {   // Hillis-Steele inclusive scan of the 1024 partial sums
        const int v = tid >= o ? part[tid - o] : 0;
        __syncthreads();
        part[tid] += v;
        __syncthreads();
    }
    int run = part[tid] - s;
    for (int i = lo; i < hi; ++i) {
        base[i] = run;
        run += count[i];
    }
    if (tid == 1023) *total = part[1023];
}

// rows [min(*total, cap), cap) of a buffer of `width` 32-bit words per row are zeroed; buf may be null
__global__ void k_mc_pad_words(unsigned* __restrict__ buf, const int* total, int cap, int width) {
    if (!buf) return;
    const size_t first = (size_t)min(max(*total, 0), cap) * width, end = (size_t)cap * width;
    for (size_t i = first + (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < end; i += (size_t)gridDim.x * blockDim.x) buf[i] = 0u;
}

// table[key] += 1 for every lane with `active`, one atomicAdd per distinct key of the wave (a body mesh has one component: 64
// lanes, one key).  Call it from wave-uniform control flow: the element-wise walks that use it (meshcc.hpp, meshorient.hpp --
// which is why it lives here) ROUND THE ELEMENT COUNT UP TO WHOLE WAVES, so that every lane of a wave reaches it and the ballots
// and shuffles together; lanes beyond the end carry active = false.
__device__ __forceinline__ void cc_add_one(int* table, int key, bool active) {
    const int lane = threadIdx.x & 63;
    unsigned long long pending = __ballot(active);
    // terminates: every round retires at least its leader, so the number of pending lanes strictly decreases and is bounded
    // below by 0; the lanes of a wave run this loop in lockstep, nobody waits
    while (pending) {
        const int leader = __ffsll((long long)pending) - 1;
        const int k = __shfl(key, leader);
        const unsigned long long same = __ballot(active && key == k);
        if (lane == leader) atomicAdd(&table[k], (int)__popcll(same));
        pending &= ~same;
    }
}

// ---- the box walkers: a face's box of n elements (pixels, cells, nodes) is walked as first, first + stride, ... < last in the
// box's row-major order by a lane (n small), by the face's wave, by one workgroup (the MEDIUM list) or by PARTS workgroups (the
// HUGE list).  The thresholds, the way the lists are appended and the per-element walk are each header's own.

// The wave's turns: every lane of the wave takes the lanes with `flagged` one after the other, lowest first; body(src) shuffles
// the source lane's set-up to itself and strides over that lane's box, first = its own lane, stride 64.
// CONTRACT: call it from wave-uniform control flow -- all 64 lanes reach the ballot together, lanes without work carry false.
template <class Body>
__device__ __forceinline__ void mesh_wave_turns(bool flagged, Body body) {
    unsigned long long todo = __ballot(flagged);
    while (todo) {   // terminates: every round clears one of at most 64 bits
        const int src = __ffsll((long long)todo) - 1;
        todo &= todo - 1;
        body(src);
    }
}

// The two lists: a one-dimensional grid of THREADS-wide workgroups strides first over the medium list, one workgroup per face,
// then over the huge list's (face, part) items, PARTS parts per face -- a face that covers everything is spread over PARTS
// workgroups.  The item and its face are the same for every thread of the workgroup.
//   size(f, ctx) -> unsigned   the elements of face f's box, 0 to skip it (an id out of range, no box); fills ctx, a Ctx of the
//                              caller's (the box: registers)
//   walk(f, ctx, first, last, stride)   the per-element work
template <int PARTS, int THREADS, class Ctx, class Size, class Walk>
__device__ __forceinline__ void mesh_list_walk(const int* __restrict__ med, unsigned n_med, const int* __restrict__ huge,
                                               unsigned n_huge, Size size, Walk walk) {
    // terminates: n_med - li strictly decreases (gridDim.x >= 1)
    for (unsigned li = blockIdx.x; li < n_med; li += gridDim.x) {
        const int f = med[li];
        Ctx ctx;
        const unsigned n = size(f, ctx);
        if (n) walk(f, ctx, threadIdx.x, n, (unsigned)THREADS);
    }
    const unsigned long long items = (unsigned long long)n_huge * PARTS;
    // terminates: items - it strictly decreases.  Item it is part it % PARTS of the face huge[it / PARTS]
    for (unsigned long long it = blockIdx.x; it < items; it += gridDim.x) {
        const int f = huge[it / PARTS];
        const unsigned part = (unsigned)(it % PARTS);
        Ctx ctx;
        const unsigned n = size(f, ctx);
        if (!n) continue;
        const unsigned per = (n + PARTS - 1) / PARTS;                     // PARTS * per >= n: the parts cover the box
        const unsigned lo = min(n, part * per), hi = min(n, lo + per);   // n < 2^31, so part * per <= n + PARTS does not wrap
        walk(f, ctx, lo + threadIdx.x, hi, (unsigned)THREADS);
    }
}

// ---- the box reduction of one workgroup of kBoxThreads threads: every thread's lo[3] / hi[3] (and flags, when sflag is not null)
// are reduced to element 0 of smin / smax / sflag, the caller's __shared__ arrays.  fmin, fmax and |= do not depend on the order.
// extra(s) is called by the threads tid < s of every round s = 128 .. 1, after the bounds and before the round's barrier: a sum
// whose order is specified rides along (k_wn_box).  CONTRACT: every thread calls it, from workgroup-uniform control flow; element 0
// may be read by every thread afterwards.
constexpr int kBoxThreads = 256;

template <class Extra>
__device__ __forceinline__ void mesh_box_reduce(const double* lo, const double* hi, int flags, double (*smin)[kBoxThreads],
                                                double (*smax)[kBoxThreads], int* sflag, Extra extra) {
    const int tid = threadIdx.x;
    for (int c = 0; c < 3; ++c) {
        smin[c][tid] = lo[c];
        smax[c][tid] = hi[c];
    }
    if (sflag) sflag[tid] = flags;
    __syncthreads();
    for (int s = kBoxThreads / 2; s > 0; s >>= 1) {
        if (tid < s) {
            for (int c = 0; c < 3; ++c) {
                smin[c][tid] = fmin(smin[c][tid], smin[c][tid + s]);
                smax[c][tid] = fmax(smax[c][tid], smax[c][tid + s]);
            }
            if (sflag) sflag[tid] |= sflag[tid + s];
            extra(s);
        }
        __syncthreads();
    }
}
