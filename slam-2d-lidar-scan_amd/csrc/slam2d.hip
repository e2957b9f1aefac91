// slam2d.hip -- gfx950 (MI355X / CDNA4) kernels + C ABI for the 2-D lidar FastSLAM hot
// path: search-field build, pose-cube sweep, arg-max / soft-max pose selection,
// occupancy-grid update, weight normalisation.  See include/slam2d.h for the
// contract and DESIGN.md for the layout and roofline of each kernel.
//
// Build: hipcc --offload-arch=gfx950 -O3 -std=c++17 -ffp-contract=off -fPIC -shared -pthread
//   -ffp-contract=off is REQUIRED: every cell index is a trunc/rint of an fp64
//   expression that sits on a lattice point, and the blur reproduces SciPy's
//   operation order; a fused multiply-add anywhere changes results.
//
// All `file:line` citations are relative to the reference repository root.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>
#include <math.h>
#include <limits.h>
#include <stdlib.h>
#include <atomic>
#include <chrono>
#include <condition_variable>
#include <mutex>
#include <thread>
#include <sched.h>
#include <stdio.h>

#include "slam2d.h"

#define WAVE 64
#define BLUR_TILE 16                 // field tile edge of the blur (power of two: BLUR_SHIFT)
#define BLUR_SHIFT 4
#define FLAG_SHIFT 3                 // occupancy flags are kept per 8 x 8-cell block (four per tile): with a blur radius of 8 the halo of
//                                      a tile is exactly its 4 x 4 blocks, so "a wall nearby" is decided exactly (3 x 3 tile flags listed
//                                      24-60 % of tiles whose halo then turned out empty)

// ------------------------------------------------------------------------------------
// stage profiling (bench.py): optional HIP-event pairs around selected kernels
// ------------------------------------------------------------------------------------
namespace {

struct StageProf {
    hipEvent_t* start = nullptr;
    hipEvent_t* stop = nullptr;
    int capacity = 0;
    int used = 0;
    int seen = 0;                    // launches of the stage since slam2d_prof_enable
};
StageProf g_prof[SLAM2D_STAGE_COUNT];
unsigned g_prof_mask = 0;
int g_prof_every = 1;                // an event pair around every g_prof_every-th launch of an enabled stage

std::mutex g_prof_mutex;             // (the groups of slam2d_groups_* may be issued from several host threads)
struct StageScope {
    int stage; hipStream_t s; int slot = -1;
    StageScope(int st, hipStream_t stream) : stage(st), s(stream) {
        if (st >= 0 && ((g_prof_mask >> st) & 1u)) {
            std::lock_guard<std::mutex> lk(g_prof_mutex);
            StageProf& p = g_prof[st];
            if (p.seen++ % g_prof_every == 0 && p.used < p.capacity) { slot = p.used++; (void)hipEventRecord(p.start[slot], s); }
        }
    }
    ~StageScope() { if (slot >= 0) (void)hipEventRecord(g_prof[stage].stop[slot], s); }
};

inline int launch_status() {
    hipError_t e = hipGetLastError();
    return e == hipSuccess ? 0 : (int)e;
}

inline int cdiv(int a, int b) { return (a + b - 1) / b; }

}  // namespace

// Phase timing inside a kernel (development aid, -DSLAM2D_DEBUG_CLOCK): thread 0 of one block stamps the
// 100 MHz wall clock at numbered points; slam2d_debug_clock() copies the stamps out.
#ifdef SLAM2D_DEBUG_CLOCK
__device__ long long g_dbg_clock[64];
#define DBG_CLOCK(i, blk) do { if ((blk) && threadIdx.x == 0) g_dbg_clock[i] = wall_clock64(); } while (0)
#else
#define DBG_CLOCK(i, blk) do { } while (0)
#endif

// ------------------------------------------------------------------------------------
// device helpers
// ------------------------------------------------------------------------------------
__device__ __forceinline__ unsigned long long order_bits(double v) {
    // monotone map double -> uint64 (so that atomicMin on the bits is a min on the values)
    unsigned long long b = (unsigned long long)__double_as_longlong(v);
    return (b & 0x8000000000000000ull) ? ~b : (b | 0x8000000000000000ull);
}
__device__ __forceinline__ double unorder_bits(unsigned long long k) {
    unsigned long long b = (k & 0x8000000000000000ull) ? (k & 0x7fffffffffffffffull) : ~k;
    return __longlong_as_double((long long)b);
}
// Block flags of one particle: [2 tmax][flag_pitch] bytes, the pitch a multiple of 16 with at least two unused (never
// written, hence never "set") bytes at the end of every row: the triage copies rows with 16-byte loads and reads the byte left
// of a row's first flag from the padding of the row above.
__host__ __device__ __forceinline__ int flag_pitch(const Slam2dLevel& lv) { return ((lv.tmax << 1) + 17) & ~15; }
__host__ __device__ __forceinline__ size_t flag_bytes(const Slam2dLevel& lv) { return (size_t)(lv.tmax << 1) * flag_pitch(lv); }
// The occupied-field image and the tile flags are not cleared between builds: a cell / tile is
// occupied when its byte equals the build's generation stamp (Slam2dLevel.occ_gen, 1..255).
__device__ __forceinline__ uint8_t occ_stamp(const Slam2dLevel& lv) { return (uint8_t)(lv.occ_gen ? lv.occ_gen : 1); }
// The needed-tile bitmap of slam2d_match: one slice per (particle, group of ep_group angles), written whole by that group's k_endpoints block
// with plain stores (every call overwrites every word: nothing to clear) and OR-ed over theta by the triage.  One shared
// bitmap per particle cost k_endpoints half of its time at 139 angles: every block's atomics met on the same few lines.
__device__ __forceinline__ int need_slices(const Slam2dLevel& lv) {
    const int G = max(lv.ep_group, 1);
    return (lv.ntheta + G - 1) / G;
}
__device__ __forceinline__ uint32_t* need_slice(const Slam2dLevel& lv, const int p, const int grp, const int nneed) {
    return lv.tileneed + ((size_t)p * need_slices(lv) + grp) * nneed;
}
// 0x01 in every byte of v that equals the stamp byte (exact per byte), 0x00 elsewhere
__device__ __forceinline__ uint32_t bytes_equal(const uint32_t v, const uint8_t stamp) {
    const uint32_t t = v ^ (0x01010101u * stamp);
    return (~(((t & 0x7f7f7f7fu) + 0x7f7f7f7fu) | t | 0x7f7f7f7fu)) >> 7;
}

// The sweep skips loads whose patch holds only the free-space constant when the cell lists are long enough to
// pay for it (k_sweep) and the tile grid fits 64-bit row masks; k_blur_check_redo then builds those masks.
__host__ __device__ __forceinline__ bool sweep_skips(const Slam2dLevel& lv) {
    return lv.freerow != nullptr && lv.tmax <= 64 && lv.kmax >= 512;
}

__device__ __forceinline__ int reflect_index(int i, int n) {
    // SciPy 'reflect' extension: d c b a | a b c d | d c b a
    int period = 2 * n;
    int m = i % period;
    if (m < 0) m += period;
    return m < n ? m : period - 1 - m;
}

// sum over the 16 lanes of a DPP row, in every lane of the row: quad butterflies, then the two mirrors (no LDS
// crossbar round trips: a ds_bpermute butterfly of 4 x 64-bit values costs ~1 us in a lone wave)
template <int CTRL>
__device__ __forceinline__ unsigned long long dpp_u64(const unsigned long long v) {
    const unsigned lo = (unsigned)__builtin_amdgcn_update_dpp(0, (int)(unsigned)v, CTRL, 0xF, 0xF, true);
    const unsigned hi = (unsigned)__builtin_amdgcn_update_dpp(0, (int)(unsigned)(v >> 32), CTRL, 0xF, 0xF, true);
    return ((unsigned long long)hi << 32) | lo;
}
__device__ __forceinline__ unsigned long long row16_sum_u64(unsigned long long t) {
    t += dpp_u64<0xB1>(t);           // quad_perm [1, 0, 3, 2]
    t += dpp_u64<0x4E>(t);           // quad_perm [2, 3, 0, 1]
    t += dpp_u64<0x141>(t);          // row_half_mirror
    t += dpp_u64<0x140>(t);          // row_mirror
    return t;
}
// u32 sum over the 16 lanes of a DPP row, in every lane
__device__ __forceinline__ unsigned row16_sum_u32(unsigned v) {
    v += (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0xB1, 0xF, 0xF, true);
    v += (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x4E, 0xF, 0xF, true);
    v += (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x141, 0xF, 0xF, true);
    v += (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x140, 0xF, 0xF, true);
    return v;
}
// the same for a double (returned as its bits): used for the 16 exp(score - M) of a tile
__device__ __forceinline__ unsigned long long row16_sum_f64(double v) {
    v += __longlong_as_double((long long)dpp_u64<0xB1>((unsigned long long)__double_as_longlong(v)));
    v += __longlong_as_double((long long)dpp_u64<0x4E>((unsigned long long)__double_as_longlong(v)));
    v += __longlong_as_double((long long)dpp_u64<0x141>((unsigned long long)__double_as_longlong(v)));
    v += __longlong_as_double((long long)dpp_u64<0x140>((unsigned long long)__double_as_longlong(v)));
    return (unsigned long long)__double_as_longlong(v);
}
// wave-wide minimum / maximum of a double without LDS round trips (all 64 lanes active): DPP inside the four rows,
// v_readlane across them
template <int CTRL>
__device__ __forceinline__ double dpp_f64(const double v) {
    return __longlong_as_double((long long)dpp_u64<CTRL>((unsigned long long)__double_as_longlong(v)));
}
__device__ __forceinline__ double readlane_f64(const double v, const int l) {
    const unsigned long long b = (unsigned long long)__double_as_longlong(v);
    const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)b, l), hi = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)(b >> 32), l);
    return __longlong_as_double((long long)(((unsigned long long)hi << 32) | lo));
}
__device__ __forceinline__ double wave64_min(double v) {
    v = fmin(v, dpp_f64<0xB1>(v)); v = fmin(v, dpp_f64<0x4E>(v)); v = fmin(v, dpp_f64<0x141>(v)); v = fmin(v, dpp_f64<0x140>(v));
    return fmin(fmin(readlane_f64(v, 0), readlane_f64(v, 16)), fmin(readlane_f64(v, 32), readlane_f64(v, 48)));
}
__device__ __forceinline__ double wave64_max(double v) {
    v = fmax(v, dpp_f64<0xB1>(v)); v = fmax(v, dpp_f64<0x4E>(v)); v = fmax(v, dpp_f64<0x141>(v)); v = fmax(v, dpp_f64<0x140>(v));
    return fmax(fmax(readlane_f64(v, 0), readlane_f64(v, 16)), fmax(readlane_f64(v, 32), readlane_f64(v, 48)));
}

// Inclusive prefix sums over the 64 lanes of a wave without LDS-crossbar round trips (a __shfl_up scan of a double is twelve
// ds_bpermute): DPP row shifts inside the four rows of 16 lanes (lanes without a source add 0), then the row totals are carried
// across with row_bcast:15 (rows 1 and 3 <- lane 15 of the row below) and row_bcast:31 (rows 2 and 3 <- lane 31).  Fixed order.
__device__ __forceinline__ double wave_scan_incl_f64(double v) {
    v += dpp_f64<0x111>(v);          // row_shr:1
    v += dpp_f64<0x112>(v);          // row_shr:2
    v += dpp_f64<0x114>(v);          // row_shr:4
    v += dpp_f64<0x118>(v);          // row_shr:8
    {
        const unsigned long long b = (unsigned long long)__double_as_longlong(v);
        const unsigned lo = (unsigned)__builtin_amdgcn_update_dpp(0, (int)(unsigned)b, 0x142, 0xA, 0xF, false);        // row_bcast:15
        const unsigned hi = (unsigned)__builtin_amdgcn_update_dpp(0, (int)(unsigned)(b >> 32), 0x142, 0xA, 0xF, false);
        v += __longlong_as_double((long long)(((unsigned long long)hi << 32) | lo));
    }
    {
        const unsigned long long b = (unsigned long long)__double_as_longlong(v);
        const unsigned lo = (unsigned)__builtin_amdgcn_update_dpp(0, (int)(unsigned)b, 0x143, 0xC, 0xF, false);        // row_bcast:31
        const unsigned hi = (unsigned)__builtin_amdgcn_update_dpp(0, (int)(unsigned)(b >> 32), 0x143, 0xC, 0xF, false);
        v += __longlong_as_double((long long)(((unsigned long long)hi << 32) | lo));
    }
    return v;
}
__device__ __forceinline__ int wave_scan_incl_i32(int v) {
    v += __builtin_amdgcn_update_dpp(0, v, 0x111, 0xF, 0xF, true);
    v += __builtin_amdgcn_update_dpp(0, v, 0x112, 0xF, 0xF, true);
    v += __builtin_amdgcn_update_dpp(0, v, 0x114, 0xF, 0xF, true);
    v += __builtin_amdgcn_update_dpp(0, v, 0x118, 0xF, 0xF, true);
    v += __builtin_amdgcn_update_dpp(0, v, 0x142, 0xA, 0xF, false);
    v += __builtin_amdgcn_update_dpp(0, v, 0x143, 0xC, 0xF, false);
    return v;
}

// (int)(v / step) -- truncation, as astype(int) -- without the fp64 division (~35 issue slots): v * (1 / step) differs from
// v / step by < 4e-16 relative, so the two truncate alike unless the quotient is within 1e-6 of an integer, where the exact
// quotient decides -- for non-negative quotients below 2^31 still WITHOUT the division when the quotient sits on an integer n, which
// is the rule, not the exception: the reference's poses stay on the map's lattice, so (coordinate - window edge) / step
// is an integer give or take an ulp for every column of the window and rounds either way: a guard that divided would send every one
// of them through the division.  (int)(v / step) is n iff the correctly rounded quotient reaches n.  r = v - n * step
// is exact as one fma (v and n * step agree in all but their last bits).  r >= 0: the real quotient is >= n, so is its rounding.
// r < 0: the quotient rounds UP to n iff it lies within half a spacing g of the doubles just below n (g = ulp(n), half that when n is
// a power of two; the tie goes to n, whose mantissa is even): r >= -(g / 2) * step, a product with a power of two, exact.
// tests/test_host_logic.py restates it in Python and checks it against the division on quotients within a few ulp of an integer.
__device__ __forceinline__ int trunc_div_fast(const double v, const double step, const double inv_step) {
    const double t = v * inv_step, n = rint(t);
    if (!(fabs(t - n) < 1e-6) && fabs(t) < 1e9) return (int)t;
    if (!(n >= 1.0 && n < 2147483648.0)) return (int)(v / step);
    const double r = __builtin_fma(-n, step, v);
    const int ni = (int)n, e = 31 - __clz(ni), pow2 = (ni & (ni - 1)) == 0 ? 1 : 0;
    const double ghalf = __longlong_as_double((long long)(1023 + e - 53 - pow2) << 52);
    return r >= -ghalf * step ? ni : ni - 1;
}

// ------------------------------------------------------------------------------------
// The exact-score core: what the sweep, tile, moments and select kernels (K1c-K1e, k_moments) share.  The project's
// invariants live here once -- the cube's shape, exact 64-bit integer cost sums, the one fp64 score expression, np.argmax's
// NaN-first order, the Slam2dMatch record.
// ------------------------------------------------------------------------------------
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));

// The pose cube of a level: nx x nx poses per angle; a plane is cut into nslot "slots" of 4 consecutive dx of one dy
// (nq per row, the last one partly padding) for the sweep and into nbt x nbt tiles of 4 x 4 poses for branch and bound,
// whose tile rows are padded to nbq4 (a multiple of 4) entries.
struct Cube { int nx, npose, nq, nslot, nbt, nbq4; };
__host__ __device__ __forceinline__ Cube cube_of(const Slam2dLevel& lv) {
    const int nx = 2 * lv.ncell + 1, nq = (nx + 3) >> 2;
    return Cube{nx, nx * nx, nq, nx * nq, nq, ((nq + 3) >> 2) << 2};
}
// Slot u of a plane: its row, first column, byte offset into a field of pitch fpitch, first pose index and valid poses
// (0 for u >= nslot, whose other members are slot 0's: safe to address with)
struct Slot { int iy, dx, off, q0, nv; };
__device__ __forceinline__ Slot slot_of(const Cube& c, const int fpitch, const int u) {
    const int uu = u < c.nslot ? u : 0;
    const int iy = uu / c.nq, dx = (uu - iy * c.nq) * 4;
    return Slot{iy, dx, (iy * fpitch + dx) * 4, iy * c.nx + dx, u < c.nslot ? min(4, c.nx - dx) : 0};
}

// Four exact 64-bit integer sums as 32-bit halves (the sum does not depend on the order: argmax ties in the reference stay ties).
// The halves are two 4-vectors, not eight scalars, on purpose: the compiler then carries them through a gather loop as two
// values, and an unrolled loop (k_moments) keeps its remainder iterations ahead of the main loop -- with scalars it moves them
// behind it and needs 83 VGPRs instead of 77, 5 waves per SIMD instead of 6, and 8 % more time for the call.
struct Acc4 {
    u32x4 lo = {0u, 0u, 0u, 0u}, hi = {0u, 0u, 0u, 0u};
    __device__ __forceinline__ void add(const u32x4 v) {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const unsigned s = lo[e] + v[e];
            hi[e] += s < v[e] ? 1u : 0u;
            lo[e] = s;
        }
    }
    __device__ __forceinline__ unsigned long long get(const int e) const { return ((unsigned long long)hi[e] << 32) | lo[e]; }
    __device__ __forceinline__ void add_u64(const int e, const unsigned long long t) {
        const unsigned long long s = get(e) + t;
        hi[e] = (unsigned)(s >> 32); lo[e] = (unsigned)s;
    }
};

// Buffer addressing (SRSRC): address = base + per-lane VGPR byte offset + wave-uniform SGPR byte offset -- no vector
// address arithmetic in a gather loop, and offsets beyond `bytes` read 0 (stores: are dropped) instead of faulting.
__device__ __forceinline__ __amdgpu_buffer_rsrc_t image_rsrc(const void* base, const size_t bytes) {
    return __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(base), (short)0, (int)bytes, 0x00020000);
}
__device__ __forceinline__ __amdgpu_buffer_rsrc_t field_rsrc(const Slam2dLevel& lv, const int p) {
    const size_t image = (size_t)lv.fmax * lv.fpitch;
    return image_rsrc(lv.field + (size_t)p * image, image * sizeof(uint32_t));
}

// Blocks of one particle are pinned to one XCD (block b runs on XCD b % 8), so that the particle's field stays in that
// XCD's 4 MiB L2: block b -> particle p (may be >= P: the grid is rounded up to 8 particles) and its w-th of `per` blocks.
__device__ __forceinline__ void xcd_particle(const int b, const int per, int* p, int* w) {
    const int xcd = b & 7, slot = b >> 3;
    *p = (slot / per) * 8 + xcd;
    *w = slot % per;
}

// The score of a pose (Utils/ScanMatcher_OGBased.py:131): its exact cost sum, rv and thetaWeight, in this association
__device__ __forceinline__ double pose_score(const unsigned long long acc, const double inv, const double prv, const double ptw) {
    return (-((double)acc * inv) + prv) + ptw;
}
// both prior planes of a slot's poses in one batch of loads (one round trip, not eight); pr: the particle's planes
__device__ __forceinline__ void slot_priors(const double* __restrict__ pr, const Cube& c, const int q0, double (&prv)[4], double (&ptw)[4]) {
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const int q = min(q0 + e, c.npose - 1);
        prv[e] = pr[q];
        ptw[e] = pr[c.npose + q];
    }
}

struct Best { double v; int i; int nan; };
__device__ __forceinline__ bool better(const Best& a, const Best& b) {
    // np.argmax semantics: first NaN wins; otherwise the largest value, lowest index on ties
    if (a.nan != b.nan) return a.nan > b.nan;
    if (a.nan) return a.i < b.i;
    return a.v > b.v || (a.v == b.v && a.i < b.i);
}
__device__ __forceinline__ Best wave_best(Best me) {
#pragma unroll
    for (int o = 1; o < WAVE; o <<= 1) {
        Best ot{__shfl_xor(me.v, o), __shfl_xor(me.i, o), __shfl_xor(me.nan, o)};
        if (better(ot, me)) me = ot;
    }
    return me;
}
__device__ __forceinline__ double wave_sum(double v) {
    // fixed order: DPP butterflies inside the four rows of 16 lanes, then (row 0 + row 1) + (row 2 + row 3) -- deterministic,
    // and no LDS-crossbar round trips (all 64 lanes must be active)
    v += dpp_f64<0xB1>(v); v += dpp_f64<0x4E>(v); v += dpp_f64<0x141>(v); v += dpp_f64<0x140>(v);
    return (readlane_f64(v, 0) + readlane_f64(v, 16)) + (readlane_f64(v, 32) + readlane_f64(v, 48));
}
// wave_best without the 6-step butterfly of three values (24 ds_bpermute) in the common case: DPP maximum, one ballot; only
// when several lanes tie for the maximum, or a NaN is present, the full comparison decides.  Same result as wave_best.  All 64
// lanes must be active.
__device__ __forceinline__ Best wave_best_fast(const Best me) {
    if (__ballot(me.nan != 0)) return wave_best(me);
    const double m = wave64_max(me.i != INT_MAX ? me.v : -INFINITY);
    const unsigned long long eq = __ballot(me.v == m && me.i != INT_MAX);
    if (!eq) return Best{-INFINITY, INT_MAX, 0};
    if ((eq & (eq - 1)) == 0ull) return Best{m, __builtin_amdgcn_readlane(me.i, __ffsll((long long)eq) - 1), 0};
    return wave_best(me);
}
// wave_best for candidates whose index ascends with the lane (so "lowest index" = lowest lane): ballots and readlanes
// instead of a 6-step butterfly of three values.  np.argmax semantics as `better`.  All 64 lanes must be active.
__device__ __forceinline__ Best wave_best_ordered(const Best me) {
    const unsigned long long nanm = __ballot(me.nan != 0);
    if (nanm) {
        const int l = __ffsll((long long)nanm) - 1;
        return Best{NAN, __builtin_amdgcn_readlane(me.i, l), 1};
    }
    const double m = wave64_max(me.v);
    const unsigned long long eq = __ballot(me.v == m && me.i != INT_MAX);
    if (!eq) return Best{-INFINITY, INT_MAX, 0};
    return Best{m, __builtin_amdgcn_readlane(me.i, __ffsll((long long)eq) - 1), 0};
}

// The Slam2dPartial of a plane, or of one 64-slot chunk of it, by one wave: lane = one slot with the scores sc[0 .. nv) (the
// lane's best of them in `me`; flat indices ascend with the lane): max / argmax in np.argmax order, sum exp(score - max).
__device__ __forceinline__ Slam2dPartial plane_partial(Best me, const double (&sc)[4], const int nv) {
    me = wave_best_ordered(me);
    double ex = 0.0;
#pragma unroll
    for (int e = 0; e < 4; ++e)
        if (e < nv) ex += exp(sc[e] - me.v);
    ex = wave_sum(ex);
    Slam2dPartial pt;
    pt.max = me.v; pt.sumexp = ex; pt.argmax = me.i; pt.has_nan = me.nan;
    return pt;
}

// A particle's nW partials to the cube's maximum and total = sum_w sumexp_w * exp(max_w - M), by one wave: `best` in
// np.argmax order; every lane owns a contiguous run of partials, whose share of the total is `mine` and whose inclusive
// scan over the lanes is `incl` (the soft-max draw walks it).  part(w): the w-th partial, however it has to be loaded.
struct PartialsTotal { Best best; double mine, incl, total; };
template <typename Load>
__device__ __forceinline__ PartialsTotal partials_total(const int nW, const Load part) {
    const int lane = threadIdx.x & 63;
    Best me{-INFINITY, INT_MAX, 0};
    for (int w = lane; w < nW; w += WAVE) {
        const Slam2dPartial pt = part(w);
        Best cand{pt.max, pt.argmax, pt.has_nan};
        if (better(cand, me)) me = cand;
    }
    me = wave_best_fast(me);
    const double M = me.v;
    const int per = (nW + WAVE - 1) / WAVE;
    const int w0 = lane * per, w1 = min(nW, w0 + per);
    double mine = 0.0;
    for (int w = w0; w < w1; ++w) { const Slam2dPartial pt = part(w); mine += pt.sumexp * exp(pt.max - M); }
    const double incl = wave_scan_incl_f64(mine);     // inclusive scan over lanes
    return PartialsTotal{me, mine, incl, readlane_f64(incl, WAVE - 1)};
}

// The match record of particle p (one lane): pose of flat cube index `pick` (theta_of_pick: its angle offset) around the
// estimate (ex, ey, eth), confidence from the maximum M and the total; then the level's arrival count.
__device__ __forceinline__ void store_match(const Slam2dLevel& lv, const int p, const double ex, const double ey, const double eth,
                                            const double theta_of_pick, const int pick, const int argmax, const double M,
                                            const double total, Slam2dMatch* out) {
    const Cube c = cube_of(lv);
    Slam2dMatch m;
    const int it = pick / c.npose, rem = pick - it * c.npose;
    const int iy = rem / c.nx, ix = rem - iy * c.nx;
    m.x = ex + (double)(ix - lv.ncell) * lv.step;                               // :142-143
    m.y = ey + (double)(iy - lv.ncell) * lv.step;
    m.theta = eth + theta_of_pick;
    m.confidence = exp(M) * total;                                              // :141
    m.log_confidence = M + log(total);
    m.best_score = M;
    m.pick = pick;
    m.argmax = argmax;
    out[p] = m;
    if (lv.arrive) __hip_atomic_fetch_add(lv.arrive, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);      // (Slam2dScan.match_seq)
}

// ------------------------------------------------------------------------------------
// The scan front end: what lies between "a pose and a scan" and "the cell lists and the occupied field"
// (Utils/ScanMatcher_OGBased.py:21-37,81-89,173-176), stated once for the kernels that need it -- a beam's angle, the
// field frame, the field index of a map column / row, occupied map bits to occupied field bytes, np.unique's hash set.
// ------------------------------------------------------------------------------------
// np.linspace(theta - fov/2, theta + fov/2, num=B) (:82-83): the last sample is the end point itself, num == 1 gives the start.
// check_level refuses fewer than 2 beams on the match and sweep paths, so in k_frame_axis and k_endpoints the one-beam case
// changes nothing reachable; it is settled per fan, not in angle(), where it cost k_endpoints<192> a second copy of its cos / sin.
struct BeamFan {
    double a0, alast, astep;           // alast: the sample of beam B - 1
    int B;
    __device__ __forceinline__ double angle(const int b) const { return (b == B - 1) ? alast : (double)b * astep + a0; }
};
__device__ __forceinline__ BeamFan fan_of(const Slam2dLidar& lid, const double theta) {
    const double a0 = theta - lid.fov / 2, a1 = theta + lid.fov / 2;
    return BeamFan{a0, lid.beams == 1 ? a0 : a1, (a1 - a0) / (double)(lid.beams - 1), lid.beams};
}

// The field frame around (ex, ey) (:22-25): its edges and its size in cells before any clamp
struct FrameExtent { double xlo, xhi, ylo, yhi; int fw, fh; };
__device__ __forceinline__ FrameExtent frame_extent(const Slam2dLevel& lv, const double ex, const double ey) {
    FrameExtent e;
    e.xlo = ex - lv.reach; e.xhi = ex + lv.reach;              // :22-23
    e.ylo = ey - lv.reach; e.yhi = ey + lv.reach;
    e.fw = (int)((e.xhi - e.xlo) / lv.step) + 1;                // :24-25
    e.fh = (int)((e.yhi - e.ylo) / lv.step) + 1;
    return e;
}
// The size of a frame record another call wrote, clipped to the slot: a frame is at most fmax x fmax, so whatever the
// record holds, no access leaves the slot's image
struct FieldSize { int fw, fh; };
__device__ __forceinline__ FieldSize frame_clip(const Slam2dLevel& lv, const Slam2dFrame& fr) {
    return FieldSize{min(fr.fw, min(lv.fmax, lv.fpitch)), min(fr.fh, lv.fmax)};
}
// What one thread per particle does at the start of a scan: the frame record, the per-scan counters, the frame's flags
__device__ __forceinline__ void frame_publish(const Slam2dLevel& lv, const int p, const Slam2dFrame& fr, const uint32_t f, uint32_t* flags) {
    lv.frames[p] = fr;
    lv.tilecount[2 * p] = 0; lv.tilecount[2 * p + 1] = 0;
    if (lv.bnb) lv.bnb_best[p] = order_bits(-INFINITY);
    if (lv.bnb >= 2) lv.seed_key[p] = 0ull;
    if (f) atomicOr(&flags[p], f);
}

// The field index of a map column / row (:32-37) from q = its (coordinate - frame edge) / step truncated as astype(int) has
// it; -1: the cell is dropped (the frame's owner raises SLAM2D_F_FIELD_INDEX).  How q is divided is the caller's choice.
__device__ __forceinline__ int axis_index(int q, const int dim) {
    if (q < 0) q += dim;                           // Python negative-index wrap (:37)
    return (q < 0 || q >= dim) ? -1 : q;
}

// Entry j of particle p's axis table -- axis 0: axis_x, the window's columns; 1: axis_y, its rows -- by the true division
// (astype(int): truncation toward zero); false where the index is out of range
__device__ __forceinline__ int axis_length(const Slam2dFrame& fr, const int axis) { return axis == 0 ? fr.mx1 - fr.mx0 : fr.my1 - fr.my0; }
__device__ __forceinline__ bool axis_table_store(const Slam2dLevel& lv, const Slam2dMap& m, const Slam2dFrame& fr, const int p,
                                                 const int axis, const int j) {
    const double d = axis == 0 ? m.X[fr.mx0 + j] - fr.xlo : m.Y[fr.my0 + j] - fr.ylo;
    const int idx = axis_index((int)(d / lv.step), axis == 0 ? fr.fw : fr.fh);
    (axis == 0 ? lv.axis_x : lv.axis_y)[(size_t)p * lv.wmax + j] = idx;
    return idx >= 0;
}

// np.unique (:120) through a hash set of cell keys in LDS (hmask + 1 slots, a power of two, INT_MAX = empty, load factor
// <= 2/3 so that an empty slot ends every probe): inserts key, gives its slot, and says whether this call was the first.
__device__ __forceinline__ bool cell_set_insert(int* hkey, const int hmask, const int key, int& slot) {
    int h = (int)(((unsigned)key * 2654435761u) >> 7) & hmask;
    for (;;) {
        const int prev = atomicCAS(&hkey[h], INT_MAX, key);
        if (prev == INT_MAX || prev == key) { slot = h; return prev == INT_MAX; }
        h = (h + 1) & hmask;
    }
}
// k_endpoints' hash set: a power of two >= 1.5 * beams, 512 at least (its LDS size is part of the launch).  No loop: as
// `while (h < n) h <<= 1` here k_endpoints<256> took 36 bytes of scratch per lane, not 20, and <192> a third spilled SGPR.
__host__ __device__ __forceinline__ int endpoints_hash_size(const int beams) {
    const int n = beams + (beams >> 1);
    return n <= 512 ? 512 : 1 << (32 - __builtin_clz(n - 1));
}

// Occupied map bits -> occupied field bytes and 8 x 8 block flags (:29-37) by one wave: lane = word w0 + lane of NR map rows
// (words[k]; fy[k]: the row's field row, wave-uniform, or -1), ax_s: the field column of every window column.  The bits of a
// non-zero word are handled by 32 lanes at once (two words per step), so a horizontal wall -- words with up to 32 bits set --
// costs one step, not 32 serial iterations of one lane.  Buffer stores: the row's byte offset rides in the scalar offset, the
// column in the lane's -- no 64-bit address arithmetic per set bit (the launch is bound by its vector instructions).
template <int NR>
__device__ __forceinline__ void scatter_expand(const Slam2dLevel& lv, const int p, const Slam2dFrame& fr, const int w0, const int lane,
                                               const uint32_t (&words)[NR], const int (&fy)[NR], const int32_t* ax_s) {
    const int col_base = (w0 + lane) << 5;
    uint32_t edge = ~0u;
    if (col_base < fr.mx0) edge &= ~0u << (fr.mx0 - col_base);                    // window edges
    if (col_base + 32 > fr.mx1) edge &= ~0u >> (col_base + 32 - fr.mx1);
    const int fpad = flag_pitch(lv);
    const __amdgpu_buffer_rsrc_t ro = image_rsrc(lv.occ + (size_t)p * lv.fmax * lv.fpitch, (size_t)lv.fmax * lv.fpitch);
    const __amdgpu_buffer_rsrc_t rt = image_rsrc(lv.tilemask + (size_t)p * flag_bytes(lv), flag_bytes(lv));   // flags of 8 x 8-cell blocks, [2 tmax][flag_pitch]
    const uint8_t stamp = occ_stamp(lv);
    const int half = lane >> 5, bit = lane & 31;
    const int lbase = (w0 << 5) + bit - fr.mx0;            // the lane's column of word w0, relative to the window
#pragma unroll
    for (int k = 0; k < NR; ++k) {
        const uint32_t word = words[k] & edge;
        unsigned long long nz = __ballot(word != 0u);
        if (!nz) continue;
        if (fy[k] < 0) continue;                                                   // :36-37
        const int so = fy[k] * lv.fpitch, st = (fy[k] >> FLAG_SHIFT) * fpad;       // (wave-uniform)
        while (nz) {
            const int sa = __ffsll((long long)nz) - 1;
            nz &= nz - 1;
            int sb = -1;
            if (nz) { sb = __ffsll((long long)nz) - 1; nz &= nz - 1; }
            // (sa, sb are wave-uniform: v_readlane, not a ds_bpermute round trip per step)
            const uint32_t wa = (uint32_t)__builtin_amdgcn_readlane((int)word, sa), wb = sb >= 0 ? (uint32_t)__builtin_amdgcn_readlane((int)word, sb) : 0u;
            const uint32_t wsel = half ? wb : wa;
            const int src = half ? sb : sa;
            if ((wsel >> bit) & 1u) {
                const int fx = ax_s[lbase + (src << 5)];
                if (fx >= 0) {
                    __builtin_amdgcn_raw_buffer_store_b8(stamp, ro, fx, so, 0);
                    __builtin_amdgcn_raw_buffer_store_b8(stamp, rt, fx >> FLAG_SHIFT, st, 0);
                }
            }
        }
    }
}

// ------------------------------------------------------------------------------------
// K2a  frame geometry                      (Utils/ScanMatcher_OGBased.py:21-28)
// ------------------------------------------------------------------------------------
// Frame geometry of one particle (every thread of k_frame_axis evaluates it redundantly: a few fp64
// operations are cheaper than a kernel boundary).
__device__ __forceinline__ Slam2dFrame make_frame(const Slam2dLidar& lid, const Slam2dLevel& lv, const Slam2dMap& m,
                                                  const double ex, const double ey, uint32_t& f) {
    const FrameExtent e = frame_extent(lv, ex, ey);
    Slam2dFrame fr;
    fr.cx = ex; fr.cy = ey;
    fr.xlo = e.xlo; fr.xhi = e.xhi; fr.ylo = e.ylo; fr.yhi = e.yhi;
    int fw = e.fw, fh = e.fh;
    f = 0;
    if (fw > lv.fmax) { fw = lv.fmax; f |= SLAM2D_F_FIELD_INDEX; }
    if (fh > lv.fmax) { fh = lv.fmax; f |= SLAM2D_F_FIELD_INDEX; }
    // checkMapToExpand (Utils/OccupancyGrid.py:108-118): the caller grows the map first
    if (fr.xlo < m.lim_x0 || fr.xhi > m.lim_x1 || fr.ylo < m.lim_y0 || fr.yhi > m.lim_y1)
        f |= SLAM2D_F_WINDOW_OUTSIDE_MAP;
    // convertRealXYToMapIdx (Utils/OccupancyGrid.py:102-106) + Python slice clipping (:29-33)
    int mx0 = (int)rint((fr.xlo - m.lim_x0) / lid.unit), mx1 = (int)rint((fr.xhi - m.lim_x0) / lid.unit);
    int my0 = (int)rint((fr.ylo - m.lim_y0) / lid.unit), my1 = (int)rint((fr.yhi - m.lim_y0) / lid.unit);
    mx0 = max(0, min(mx0, m.cols)); mx1 = max(mx0, min(mx1, m.cols));
    my0 = max(0, min(my0, m.rows)); my1 = max(my0, min(my1, m.rows));
    if (mx1 - mx0 > lv.wmax) { mx1 = mx0 + lv.wmax; f |= SLAM2D_F_WINDOW_OUTSIDE_MAP; }
    if (my1 - my0 > lv.wmax) { my1 = my0 + lv.wmax; f |= SLAM2D_F_WINDOW_OUTSIDE_MAP; }
    fr.fh = fh; fr.fw = fw; fr.mx0 = mx0; fr.mx1 = mx1; fr.my0 = my0; fr.my1 = my1;
    fr.field_min = lv.floor_value; fr.redo = 0; fr.min_known = 0;
    fr.field_max = 0.0;
    return fr;
}

// ------------------------------------------------------------------------------------
// K2a+b  frame geometry (:21-28) and the field index of every window column / row (:32-36,173-176)
// ------------------------------------------------------------------------------------
__global__ void k_frame_axis(Slam2dLidar lid, Slam2dLevel lv, const Slam2dMap* __restrict__ maps,
                             const double* __restrict__ centre, int cstride, uint32_t* flags,
                             const double* __restrict__ ranges) {
    const int p = blockIdx.y, axis = blockIdx.z;
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    if (ranges && axis == 0) {
        // covertMeasureToXY (Utils/ScanMatcher_OGBased.py:81-89) once per particle: k_endpoints' ntheta blocks of the
        // particle would otherwise each evaluate the same cos / sin (a third of its time at 1081 beams x 139 angles)
        const double ex = centre[(size_t)p * cstride], ey = centre[(size_t)p * cstride + 1], eth = centre[(size_t)p * cstride + 2];
        const int B = lid.beams;
        const BeamFan fan = fan_of(lid, eth);
        for (int b = j; b < B; b += gridDim.x * blockDim.x) {
            const double rg = ranges[b];
            const double a = fan.angle(b);
            lv.beam_xy[((size_t)p * B + b) * 2] = ex + cos(a) * rg;                              // :87
            lv.beam_xy[((size_t)p * B + b) * 2 + 1] = ey + sin(a) * rg;                          // :88
        }
    }
    const Slam2dMap m = maps[p];
    uint32_t f;
    const Slam2dFrame fr = make_frame(lid, lv, m, centre[(size_t)p * cstride], centre[(size_t)p * cstride + 1], f);
    if (j == 0 && axis == 0) frame_publish(lv, p, fr, f, flags);
    if (j < axis_length(fr, axis) && !axis_table_store(lv, m, fr, p, axis, j)) atomicOr(&flags[p], SLAM2D_F_FIELD_INDEX);
}

// ------------------------------------------------------------------------------------
// K2c  occupied map cells -> occupied field cells  (Utils/ScanMatcher_OGBased.py:29-37)
//      HBM-bound: streams the map window once (4 B / map cell), byte scatter into occ.
// ------------------------------------------------------------------------------------
// The occupied / free state of every map cell is kept as one bit (Slam2dMap.occ_bits, maintained by
// the update kernel), so the field build reads 1/32 of the bytes the count map holds.
// One thread = one 32-cell word of the map window.
#define SCATTER_ROWS 32
__global__ __launch_bounds__(256) void k_occ_scatter(Slam2dLevel lv, const Slam2dMap* __restrict__ maps) {
    // wave = threadIdx.y walks 8 rows of the map window; lane = one 32-cell word of the row (scatter_expand)
    const int p = blockIdx.z;
    const Slam2dFrame fr = lv.frames[p];
    const int nrow = fr.my1 - fr.my0;
    if (fr.mx1 <= fr.mx0 || nrow <= 0) return;
    const int lane = threadIdx.x, wave = threadIdx.y;
    const int w0 = (fr.mx0 >> 5) + blockIdx.x * 64, wlast = (fr.mx1 - 1) >> 5;
    if (w0 > wlast) return;
    const int w = w0 + lane;
    const Slam2dMap m = maps[p];
    constexpr int NR = SCATTER_ROWS / 4;
    const int i0 = blockIdx.y * SCATTER_ROWS + wave;
    // the field column of every window column is staged in LDS and the rows' field indices are loaded with
    // the words: the expansion loop below then has no global load in its dependency chain
    extern __shared__ int32_t ax_s[];
    {
        const int32_t* __restrict__ ax = lv.axis_x + (size_t)p * lv.wmax;
        for (int j = wave * 64 + lane; j < axis_length(fr, 0); j += 256) ax_s[j] = ax[j];
    }
    uint32_t words[NR];
    int fyk[NR];
#pragma unroll
    for (int k = 0; k < NR; ++k) {
        const int i = i0 + 4 * k;
        words[k] = (i < nrow && w <= wlast) ? m.occ_bits[(size_t)(fr.my0 + i) * m.bits_pitch + w] : 0u;
        fyk[k] = i < nrow ? lv.axis_y[(size_t)p * lv.wmax + i] : -1;
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < NR; ++k) fyk[k] = __builtin_amdgcn_readfirstlane(fyk[k]);  // (the wave's row: uniform)
    scatter_expand<NR>(lv, p, fr, w0, lane, words, fyk, ax_s);
}

// k_occ_scatter's work as a block role of k_endpoints' launch (slam2d_match below 512 beams, where no k_frame_axis
// precedes it): the block derives the frame itself and evaluates the field index of its columns / rows inline (:32-37)
// instead of reading the axis tables the frame block of the same launch is still writing.  Block (sbx, sby) of NW waves:
// wave = SCATTER_ROLE_NR rows of the map window, lane = one 32-cell word.  Out-of-range indices are skipped here and
// flagged by the frame block.
#ifndef SCATTER_ROLE_NR
#define SCATTER_ROLE_NR 8           // map rows per wave of the scatter role (every block derives the field index of ALL window columns first)
#endif
template <int NW>
__device__ __forceinline__ void scatter_role(const Slam2dLidar& lid, const Slam2dLevel& lv, const Slam2dMap* __restrict__ maps,
                                             const double* __restrict__ centre, const int cstride, const int p,
                                             const int sbx, const int sby, int32_t* ax_s) {
    const Slam2dMap m = maps[p];
    uint32_t fignore;
    const Slam2dFrame fr = make_frame(lid, lv, m, centre[(size_t)p * cstride], centre[(size_t)p * cstride + 1], fignore);
    const int nrow = fr.my1 - fr.my0;
    if (fr.mx1 <= fr.mx0 || nrow <= 0) return;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int w0 = (fr.mx0 >> 5) + sbx * 64, wlast = (fr.mx1 - 1) >> 5;
    if (w0 > wlast) return;
    const int w = w0 + lane;
    constexpr int NR = SCATTER_ROLE_NR;
    const int i0 = sby * (NW * NR) + wave;
    if (sby * (NW * NR) >= nrow) return;
    const double inv_step = 1.0 / lv.step;
    // (the rows' words and coordinates are requested FIRST: they need the frame only, and their round trip then runs under the
    // column table's)
    uint32_t words[NR];
    int fyk[NR];
#pragma unroll
    for (int k = 0; k < NR; ++k) {
        const int i = i0 + NW * k;
        words[k] = (i < nrow && w <= wlast) ? m.occ_bits[(size_t)(fr.my0 + i) * m.bits_pitch + w] : 0u;
    }
    const double ycoord = (lane < NR && i0 + NW * lane < nrow) ? m.Y[fr.my0 + i0 + NW * lane] : 0.0;
    for (int j = threadIdx.x; j < axis_length(fr, 0); j += NW * 64)
        ax_s[j] = axis_index(trunc_div_fast(m.X[fr.mx0 + j] - fr.xlo, lv.step, inv_step), fr.fw);
    int fy_lane = -1;                                      // lane k < NR evaluates the field row of the wave's k-th map row
    if (lane < NR && i0 + NW * lane < nrow) fy_lane = axis_index(trunc_div_fast(ycoord - fr.ylo, lv.step, inv_step), fr.fh);
#pragma unroll
    for (int k = 0; k < NR; ++k) fyk[k] = __builtin_amdgcn_readlane(fy_lane, k);
    __syncthreads();
    scatter_expand<NR>(lv, p, fr, w0, lane, words, fyk, ax_s);
}

// ------------------------------------------------------------------------------------
// K2d  exact squared Euclidean distance to the nearest occupied field cell, clamped at cap = lut_n - 1, through a table
//      (slam2d_field_build_distance).  Integers only; every join is a minimum.
// ------------------------------------------------------------------------------------
// The result is clamped at cap <= R * R, R = ceil(sqrt(cap)): a cell whose answer is below the cap has its nearest wall fewer
// than R rows AND fewer than R columns away, so both passes of the separable transform look R cells far and no farther, and a
// column distance saturated at R + 1 -- (R + 1)^2 > cap -- stands for "none in reach".
//
// Column pass: g(i, j) = rows from (i, j) to the nearest occupied cell of column j, saturated at R + 1, into the slot's field
// image.  One thread = one column of a segment of S rows: down from R rows above the segment, then up from R rows below it, so
// a thread writes only its own segment and reads nothing another thread writes.
__global__ __launch_bounds__(256) void k_dist_cols(Slam2dLevel lv, const int R, const int S) {
    const int p = blockIdx.z;
    const FieldSize fs = frame_clip(lv, lv.frames[p]);
    const int j = blockIdx.x * 256 + threadIdx.x, r0 = blockIdx.y * S, r1 = min(r0 + S, fs.fh);
    if (j >= fs.fw || r0 >= fs.fh) return;
    const uint8_t* __restrict__ occ = lv.occ + (size_t)p * lv.fmax * lv.fpitch + j;
    uint32_t* g = lv.field + (size_t)p * lv.fmax * lv.fpitch + j;
    const uint8_t stamp = occ_stamp(lv);
    const int sat = R + 1;
    int d = sat;
#pragma unroll 4
    for (int a = max(0, r0 - R); a < r1; ++a) {
        d = occ[a * lv.fpitch] == stamp ? 0 : min(d + 1, sat);
        if (a >= r0) g[a * lv.fpitch] = (uint32_t)d;
    }
    d = sat;
#pragma unroll 4
    for (int a = min(fs.fh, r1 + R) - 1; a >= r0; --a) {
        d = occ[a * lv.fpitch] == stamp ? 0 : min(d + 1, sat);
        if (a < r1 && (uint32_t)d < g[a * lv.fpitch]) g[a * lv.fpitch] = (uint32_t)d;
    }
}

// Row pass: k(i, j) = min(cap, min over |b - j| <= R of (b - j)^2 + g(i, b)^2); field = lut[k], dist2 = k.  One block = one
// row: the row of g goes from the field image into LDS as 16-bit values (0 .. 257; fmax <= 23170: 46 KB) before the block
// overwrites it, so no block reads what another one writes.  A cell stops at the offset whose square reaches its minimum so
// far; a row without a wall in reach of any of its cells is the cap throughout.
__global__ __launch_bounds__(256) void k_dist_rows(Slam2dLevel lv, const uint32_t* __restrict__ lut, const int cap, const int R,
                                                   uint32_t* __restrict__ dist2) {
    extern __shared__ __attribute__((aligned(16))) uint16_t dist_g_s[];
    const int p = blockIdx.y, i = blockIdx.x;
    const FieldSize fs = frame_clip(lv, lv.frames[p]);
    if (i >= fs.fh) return;                                // (the whole block)
    const size_t row = ((size_t)p * lv.fmax + i) * lv.fpitch;
    uint32_t* f = lv.field + row;
    int near = 0;
    for (int j = threadIdx.x; j < fs.fw; j += 256) {
        const uint32_t g = min(f[j], (uint32_t)(R + 1));
        dist_g_s[j] = (uint16_t)g;
        near |= g <= (uint32_t)R ? 1 : 0;
    }
    const int any = __syncthreads_or(near);
    for (int j = threadIdx.x; j < fs.fw; j += 256) {
        int best = cap;
        if (any) {
            const int g0 = dist_g_s[j];
            best = min(best, g0 * g0);
            for (int o = 1; o * o < best; ++o) {
                if (j - o >= 0) { const int g = dist_g_s[j - o]; best = min(best, o * o + g * g); }
                if (j + o < fs.fw) { const int g = dist_g_s[j + o]; best = min(best, o * o + g * g); }
            }
        }
        f[j] = lut[best];
        if (dist2) dist2[row + j] = (uint32_t)best;
    }
}

__global__ __launch_bounds__(256) void k_refresh_bits(const Slam2dMap* __restrict__ maps, const int32_t* __restrict__ index) {
    // one wave = 64 consecutive cells of a row: coalesced 256-byte read, one ballot, two words out
    const Slam2dMap m = maps[index ? index[blockIdx.y] : blockIdx.y];
    const int lane = threadIdx.x & 63;
    const int groups_per_row = (m.cols + 63) >> 6;
    const long long ngroups = (long long)m.rows * groups_per_row;
    for (long long g = (long long)blockIdx.x * 4 + (threadIdx.x >> 6); g < ngroups; g += (long long)gridDim.x * 4) {
        const int row = (int)(g / groups_per_row), c0 = (int)(g - (long long)row * groups_per_row) << 6;
        const int col = c0 + lane;
        bool occ = false;
        if (col < m.cols) {
            if (m.wide) {
                const unsigned long long v = reinterpret_cast<const unsigned long long*>(m.cells)[(size_t)row * m.pitch + col];
                occ = 2ull * (v >> 32) > (v & 0xffffffffull);
            } else {
                const uint32_t v = m.cells[(size_t)row * m.pitch + col];
                occ = 2u * (v >> 16) > (v & 0xffffu);                              // :29-31
            }
        }
        const unsigned long long mask = __ballot(occ);
        if (lane < 2 && (c0 >> 5) + lane < m.bits_pitch)
            m.occ_bits[(size_t)row * m.bits_pitch + (c0 >> 5) + lane] = (uint32_t)(mask >> (32 * lane));
    }
}

// ------------------------------------------------------------------------------------
// K2d  separable Gaussian blur + clamp           (Utils/ScanMatcher_OGBased.py:41-45)
//      fp64, SciPy's symmetric correlate1d operation order, axis 0 then axis 1,
//      'reflect' borders.  The clamp threshold is 0.5 * (field minimum); the minimum
//      is known analytically (floor_value) whenever some cell has an all-free
//      neighbourhood, which k_blur_check_redo verifies from the measured minimum and
//      mode 1 redoes the clamp with the measured minimum otherwise.
// ------------------------------------------------------------------------------------
#define BLUR_THREADS 64              // one wave per tile: no cross-wave barriers
#define SLAM2D_BLUR_BLOCKS_PER_PARTICLE 256
#define BLUR_EXT (BLUR_TILE + 2 * SLAM2D_MAX_BLUR_RADIUS)
// RAD > 0: radius known at compile time, RAD <= 8 (register sliding windows, fully unrolled, LDS sized
// for it); RAD == 0: any radius up to SLAM2D_MAX_BLUR_RADIUS (loops over LDS).
//
// Work avoidance (all bit-exact):
//  * a tile whose halo holds no occupied cell is all "free": every value equals the analytic
//    floor, so it is filled with that constant without arithmetic;
//  * lv.tilestate remembers, across scans, which tiles of the (reused) field buffer already
//    hold that constant: a tile that was free at the previous build and is free now is not
//    touched at all -- the field build then costs HBM traffic only where walls are.
// Tiles are 16x16: walls are thin, so small tiles keep the blurred area close to the area that
// actually differs from the constant (work ~ (T + 2r + 1) * (2 + 2r/T) per unit wall length has its
// minimum near T = 2r).
//
// The tile body is one wave's work (k_blur_clamp's blocks are one wave; k_blur_check_redo's redo runs in its first wave alone):
// a vote over the tile is a ballot, not a block reduction.
__device__ __forceinline__ int blur_wave_any(const int pred) { return __ballot(pred != 0) != 0ull; }
// base + a 32-bit BYTE offset: the address is a uniform base and one vector register (offsets into one particle's image,
// field or block minima stay below 2^31: fmax * fpitch < 2^29 is checked at every entry point)
template <typename T>
__device__ __forceinline__ T* at_bytes(T* base, const uint32_t byte_offset) {
    using B = std::conditional_t<std::is_const_v<T>, const char, char>;
    return reinterpret_cast<T*>(reinterpret_cast<B*>(base) + byte_offset);
}
// 0x01 in every byte of v that differs from the stamp byte (exact per byte), 0x00 where it equals it
__device__ __forceinline__ uint32_t bytes_differ(const uint32_t v, const uint8_t stamp) {
    const uint32_t t = v ^ (0x01010101u * stamp);
    return ((((t & 0x7f7f7f7fu) + 0x7f7f7f7fu) | t) >> 7) & 0x01010101u;
}
// reflect_index for an index within one length of the range (every halo of a frame that is not smaller than the radius): two
// selects; anything further out takes the general form with its division
__device__ __forceinline__ int reflect_near(const int i, const int n) {
    int m = i < 0 ? -1 - i : i;
    m = m >= n ? 2 * n - 1 - m : m;
    if (__builtin_expect((unsigned)m >= (unsigned)n, 0)) m = reflect_index(i, n);
    return m;
}
// Slice i of a PER_ROW-wide array of TOTAL elements dealt over the wave, 64 at a time: the lane's (row, column).  Where the
// wave covers whole rows the column is the lane's own in every slice and the rows are a constant apart (addresses differ by
// immediates); a last, partial slice is clamped into the array (its lanes beyond the end are masked by blur_slice_valid).
template <int PER_ROW, int TOTAL>
__device__ __forceinline__ void blur_slice(const int tid, const int i, int& row, int& col) {
    if constexpr (BLUR_THREADS % PER_ROW == 0) {
        row = tid / PER_ROW + i * (BLUR_THREADS / PER_ROW);
        col = tid % PER_ROW;
        if ((i + 1) * BLUR_THREADS > TOTAL) row = min(row, TOTAL / PER_ROW - 1);
    } else {
        int idx = tid + i * BLUR_THREADS;
        if ((i + 1) * BLUR_THREADS > TOTAL) idx = min(idx, TOTAL - 1);
        row = idx / PER_ROW;
        col = idx - row * PER_ROW;
    }
}
template <int TOTAL>
__device__ __forceinline__ bool blur_slice_valid(const int tid, const int i) {
    return (i + 1) * BLUR_THREADS <= TOTAL || tid + i * BLUR_THREADS < TOTAL;
}
// The blur weights are uniform and constant for the launch: read through the constant address space they are scalar loads and
// the taps take them from scalar registers.
typedef const double __attribute__((address_space(4))) * BlurWeights;
template <int RAD>
struct BlurLds {
    static constexpr int EXT = RAD > 0 ? BLUR_TILE + 2 * RAD : BLUR_EXT;
    uint8_t occ[EXT][EXT + 4];
    double mid[BLUR_TILE][EXT + 5];        // pitch 37 doubles at RAD = 8: conflict-free b64 row reads
    double red;
};

template <int RAD>
__device__ __forceinline__ void blur_tile(const Slam2dLevel& lv, BlurLds<RAD>& sm, const int p, const Slam2dFrame& fr,
                                          const int tby, const int tbx, const int mode, const bool use_flags,
                                          const bool minmax = true) {
    // minmax == false (mode 0 only): the caller knows that nobody will read this build's tilemin / tilemax -- the tile's two wave
    // reductions and their stores are skipped
    const int fh = fr.fh, fw = fr.fw;
    const int ty0 = tby * BLUR_TILE, tx0 = tbx * BLUR_TILE;
    if (ty0 >= fh || tx0 >= fw) return;
    const int r = RAD > 0 ? RAD : lv.blur_radius;
    const int ext = BLUR_TILE + 2 * r;
    const int tid = threadIdx.x;
    const bool dbg = p == 0 && blockIdx.x == 0 && mode == 0;
    DBG_CLOCK(50, dbg);
    const uint8_t* occ = lv.occ + (size_t)p * lv.fmax * lv.fpitch;
    const uint8_t stamp = occ_stamp(lv);
    uint8_t* state = lv.tilestate + ((size_t)p * lv.tmax + tby) * lv.tmax + tbx;
    // activity: an occupied cell within the halo lies in one of the 8 x 8-cell blocks within ceil(r / 8) blocks of the tile's four
    int any = 1;
    if (use_flags) {
        any = 0;
        const uint8_t* tiles = lv.tilemask + (size_t)p * flag_bytes(lv);
        const int nsy = (fh + 7) >> FLAG_SHIFT, nsx = (fw + 7) >> FLAG_SHIFT, k = (r + 7) >> FLAG_SHIFT, e = 2 + 2 * k;
        if (tid < e * e) {
            const int yy = 2 * tby - k + tid / e, xx = 2 * tbx - k + tid % e;
            if (yy >= 0 && yy < nsy && xx >= 0 && xx < nsx) any = tiles[yy * flag_pitch(lv) + xx] == stamp;
        }
        any = blur_wave_any(any);
    }
    if (any) {
        // word loads when the halo is interior and 4-byte aligned (r % 4 == 0), bytes + reflect otherwise
        const bool interior = ty0 - r >= 0 && ty0 + BLUR_TILE + r <= fh && tx0 - r >= 0 && tx0 + BLUR_TILE + r <= fw;
        int exact = 0;                 // the tile flags are conservative: re-test on the halo itself
        // every load of the halo is issued before the first use: the image is not cache-resident (one
        // HBM latency instead of one per 64-lane slice)
        if ((r & 3) == 0 && interior) {
            const int wpr = ext >> 2;
            if constexpr (RAD > 0) {
                // the address is the particle's image (uniform) plus a 32-bit byte offset (fmax * fpitch < 2^29)
                constexpr int WPR = (BLUR_TILE + 2 * RAD) / 4, TOTAL = (BLUR_TILE + 2 * RAD) * WPR;
                constexpr int NW = (TOTAL + BLUR_THREADS - 1) / BLUR_THREADS;
                uint32_t v[NW];
#pragma unroll
                for (int i = 0; i < NW; ++i) {
                    int ly, lw;
                    blur_slice<WPR, TOTAL>(tid, i, ly, lw);
                    v[i] = *at_bytes(reinterpret_cast<const uint32_t*>(occ), (uint32_t)((ty0 - RAD + ly) * lv.fpitch + (tx0 - RAD) + 4 * lw));
                }
                uint32_t all_free = 0x01010101u;
#pragma unroll
                for (int i = 0; i < NW; ++i) {
                    if (blur_slice_valid<TOTAL>(tid, i)) {
                        int ly, lw;
                        blur_slice<WPR, TOTAL>(tid, i, ly, lw);
                        const uint32_t f = bytes_differ(v[i], stamp);                                        // (RAD > 0: the LDS image holds 1 = free)
                        *reinterpret_cast<uint32_t*>(&sm.occ[ly][4 * lw]) = f;
                        all_free &= f;
                    }
                }
                exact = all_free != 0x01010101u;                                                             // one test for the lane's words
            } else {
                for (int idx = tid; idx < ext * wpr; idx += BLUR_THREADS) {
                    const int ly = idx / wpr, lw = idx - ly * wpr;
                    const uint32_t v = bytes_equal(*reinterpret_cast<const uint32_t*>(occ + (size_t)(ty0 - r + ly) * lv.fpitch + (tx0 - r) + 4 * lw), stamp);
                    *reinterpret_cast<uint32_t*>(&sm.occ[ly][4 * lw]) = v;
                    exact |= (v != 0u);
                }
            }
        } else if constexpr (RAD > 0) {
            constexpr int EXT_C = BLUR_TILE + 2 * RAD;
            constexpr int NB = (EXT_C * EXT_C + BLUR_THREADS - 1) / BLUR_THREADS;
            uint8_t v[NB];
#pragma unroll
            for (int i = 0; i < NB; ++i) {
                int ly, lx;
                blur_slice<EXT_C, EXT_C * EXT_C>(tid, i, ly, lx);
                const int gy = reflect_near(ty0 - r + ly, fh), gx = reflect_near(tx0 - r + lx, fw);
                v[i] = *at_bytes(occ, (uint32_t)(gy * lv.fpitch + gx));
            }
#pragma unroll
            for (int i = 0; i < NB; ++i) {
                if (blur_slice_valid<EXT_C * EXT_C>(tid, i)) {
                    int ly, lx;
                    blur_slice<EXT_C, EXT_C * EXT_C>(tid, i, ly, lx);
                    const uint8_t o = v[i] == stamp;
                    sm.occ[ly][lx] = o ^ 1;
                    exact |= o;
                }
            }
        } else {
            for (int idx = tid; idx < ext * ext; idx += BLUR_THREADS) {
                const int ly = idx / ext, lx = idx - ly * ext;
                const int gy = reflect_index(ty0 - r + ly, fh), gx = reflect_index(tx0 - r + lx, fw);
                const uint8_t o = occ[(size_t)gy * lv.fpitch + gx] == stamp;
                sm.occ[ly][lx] = o;
                exact |= o;
            }
        }
        __syncthreads();                               // the image is in LDS
        any = blur_wave_any(exact);
    }
    DBG_CLOCK(51, dbg);
    const double L = lv.log_miss;
    const double fmin_used = mode == 1 ? fr.field_min : lv.floor_value;
    const double thr = 0.5 * fmin_used;                                            // :44
    uint32_t* field = lv.field + (size_t)p * lv.fmax * lv.fpitch;
    const double* __restrict__ w = lv.blur_w;
    const BlurWeights wc = (BlurWeights)(uintptr_t)lv.blur_w;                      // (RAD > 0)
    if (!any) {
        const double v = lv.floor_value;
        if (mode == 0 && minmax && tid == 0) {
            lv.tilemin[((size_t)p * lv.tmax + tby) * lv.tmax + tbx] = v;
            lv.tilemax[((size_t)p * lv.tmax + tby) * lv.tmax + tbx] = v > thr ? 0.0 : v;
        }
        if (mode == 0 && *state == 0) return;          // already holds the constant: nothing to write
        const uint32_t c = v > thr ? 0u : (uint32_t)rint(-v * lv.cost_scale);
        for (int idx = tid; idx < BLUR_TILE * BLUR_TILE; idx += BLUR_THREADS) {
            const int y = idx / BLUR_TILE, x = idx - y * BLUR_TILE;
            if (tx0 + x < lv.fpitch && ty0 + y < lv.fmax) field[(size_t)(ty0 + y) * lv.fpitch + tx0 + x] = c;
            // the tile's 4 x 4 block minima, from inside this loop (a separate store after it costs the kernel 17
            // VGPRs and a third of its waves)
            if (lv.bnb && ((y | x) & 3) == 0) lv.gmin[((size_t)p * (lv.tmax << 2) + ((ty0 + y) >> 2)) * (lv.tmax << 2) + ((tx0 + x) >> 2)] = c;
        }
        if (tid == 0) *state = mode == 0 ? 0 : 1;
        return;
    }
    if (tid == 0) *state = 1;
    double lmin = INFINITY, lmax = -INFINITY;     // of the blurred values / of the values as stored (after the clamp)
    // SciPy symmetric correlate1d order: out = a[c]*w[c]; for j=-r..-1: out += (a[c+j] + a[c-j]) * w[j]
    if constexpr (RAD > 0) {
        {   // axis-0 pass: lane = (column lx, half of the tile's rows: 8 consecutive outputs)
            constexpr int EXT_C = BLUR_TILE + 2 * RAD;
            static_assert(2 * EXT_C <= BLUR_THREADS, "one wave covers the axis-0 pass only for RAD <= 8");
            const int lx = tid % EXT_C, g = tid / EXT_C;
            if (g < 2) {
                // The inputs are 0.0 (occupied) or L, so a tap's pair sum is 0, L or 2L and its product with the weight is 0, L w or
                // 2 (L w) EXACTLY: with f = 0 / 1 and lw = L * w the tap is fma(f_a + f_b, lw, acc) -- the product inside is exact,
                // the one rounding is the sum's, as in SciPy's acc + (a + b) * w -- two operations instead of three.  (The centre term
                // is selected, not multiplied: 0.0 * lw would be -0.0.)
                // The centre term is fma(f, lw, +0.0): lw + 0.0 = lw for a free cell, (-0.0) + (+0.0) = +0.0 for an occupied one -- the
                // value a select gives, in one operation (0.0 * lw alone would be -0.0).
                // One conversion per value (1 = free -> 1.0), both words of the double at once; the kernel's register bound (four
                // waves per SIMD, k_blur_clamp) keeps the scheduler from holding all of them at once with everything else.
                double f[8 + 2 * RAD], lw[RAD + 1];
#pragma unroll
                for (int k = 0; k < 8 + 2 * RAD; ++k) f[k] = (double)(uint32_t)sm.occ[g * 8 + k][lx];
#pragma unroll
                for (int j = 0; j <= RAD; ++j) lw[j] = L * wc[j];
#pragma unroll
                for (int o = 0; o < 8; ++o) {
                    double acc = __builtin_fma(f[o + RAD], lw[RAD], 0.0);
#pragma unroll
                    for (int j = -RAD; j < 0; ++j) acc = __builtin_fma(f[o + RAD + j] + f[o + RAD - j], lw[RAD + j], acc);
                    sm.mid[g * 8 + o][lx] = acc;
                }
            }
        }
        __syncthreads();
        DBG_CLOCK(52, dbg);
        {   // axis-1 pass: lane = (row y, 4 consecutive columns)
            const int y = tid >> 2, x0 = (tid & 3) * 4;
            double mrow[4 + 2 * RAD];
#pragma unroll
            for (int k = 0; k < 4 + 2 * RAD; ++k) mrow[k] = sm.mid[y][x0 + k];
            // The four values and their costs are computed for every lane (the LDS rows hold reflected values beyond the frame); the
            // frame decides only what is stored and what enters the minima: ONE test per lane where its quad lies inside the frame
            // (a 16-byte store, as fill_tile's), the per-cell tests for a frame's last columns.
            double acc[4];
            uint32_t cst[4];
#pragma unroll
            for (int o = 0; o < 4; ++o) {
                double a = mrow[o + RAD] * wc[RAD];
#pragma unroll
                for (int j = -RAD; j < 0; ++j) a = a + (mrow[o + RAD + j] + mrow[o + RAD - j]) * wc[RAD + j];
                acc[o] = a;
                cst[o] = a > thr ? 0u : (uint32_t)rint(-a * lv.cost_scale);
            }
            const int gy = ty0 + y, gx = tx0 + x0;
            const bool row_in = gy < fh;
            const uint32_t cell = (uint32_t)(gy * lv.fpitch + gx);
            uint32_t cmin = 0xffffffffu;                   // of the lane's 4 stored costs: one row of an aligned 4x4 block
            if (row_in && gx + 3 < fw) {
                *reinterpret_cast<uint4*>(at_bytes(field, 4u * cell)) = make_uint4(cst[0], cst[1], cst[2], cst[3]);
                cmin = min(min(cst[0], cst[1]), min(cst[2], cst[3]));
            } else if (row_in) {
#pragma unroll
                for (int o = 0; o < 4; ++o)
                    if (gx + o < fw) {
                        *at_bytes(field, 4u * (cell + o)) = cst[o];
                        cmin = min(cmin, cst[o]);
                    }
            }
            if (mode == 0 && minmax) {                     // (uniform: the minima of the values are read by the minimum check alone)
#pragma unroll
                for (int o = 0; o < 4; ++o)
                    if (row_in && gx + o < fw) {
                        lmin = fmin(lmin, acc[o]);
                        lmax = fmax(lmax, acc[o]);         // (clamped after the loop: the clamp is monotone)
                    }
                if (lmax > thr) lmax = 0.0;
            }
            if (lv.bnb) {                                  // rows y, y^1, y^2, y^3 of the block sit in lanes tid ^ 4, ^ 8
                cmin = min(cmin, (uint32_t)__builtin_amdgcn_update_dpp(-1, (int)cmin, 0x124, 0xF, 0xF, false));   // row_ror:4
                cmin = min(cmin, (uint32_t)__builtin_amdgcn_update_dpp(-1, (int)cmin, 0x128, 0xF, 0xF, false));   // row_ror:8
                if ((y & 3) == 0) {
                    const int gp = lv.tmax << 2;
                    uint32_t* gmin = lv.gmin + (size_t)p * gp * gp;
                    *at_bytes(gmin, 4u * (uint32_t)(((ty0 >> 2) + (y >> 2)) * gp + (tx0 >> 2) + (tid & 3))) = cmin;
                }
            }
        }
    } else {
        for (int idx = tid; idx < BLUR_TILE * ext; idx += BLUR_THREADS) {
            const int y = idx / ext, lx = idx - y * ext;
            double acc = (sm.occ[y + r][lx] ? 0.0 : L) * w[r];
            for (int j = -r; j < 0; ++j) {
                const double a = sm.occ[y + r + j][lx] ? 0.0 : L;
                const double b = sm.occ[y + r - j][lx] ? 0.0 : L;
                acc = acc + (a + b) * w[r + j];
            }
            sm.mid[y][lx] = acc;
        }
        __syncthreads();
        for (int idx = tid; idx < BLUR_TILE * BLUR_TILE; idx += BLUR_THREADS) {
            const int y = idx / BLUR_TILE, x = idx - y * BLUR_TILE;
            double acc = sm.mid[y][x + r] * w[r];
            for (int j = -r; j < 0; ++j) acc = acc + (sm.mid[y][x + r + j] + sm.mid[y][x + r - j]) * w[r + j];
            const int gy = ty0 + y, gx = tx0 + x;
            uint32_t cmin = 0xffffffffu;
            if (gy < fh && gx < fw) {
                lmin = fmin(lmin, acc);
                lmax = fmax(lmax, acc > thr ? 0.0 : acc);
                cmin = acc > thr ? 0u : (uint32_t)rint(-acc * lv.cost_scale);
                field[(size_t)gy * lv.fpitch + gx] = cmin;
            }
            if (lv.bnb) {        // this pass covers rows 4i .. 4i+3 (i = idx / 64): lane = (row tid >> 4, column tid & 15)
                cmin = min(cmin, (uint32_t)__shfl_xor((int)cmin, 1));
                cmin = min(cmin, (uint32_t)__shfl_xor((int)cmin, 2));
                cmin = min(cmin, (uint32_t)__shfl_xor((int)cmin, 16));
                cmin = min(cmin, (uint32_t)__shfl_xor((int)cmin, 32));
                if ((tid & 0x33) == 0) {
                    const int gp = lv.tmax << 2;
                    lv.gmin[((size_t)p * gp + (ty0 >> 2) + (idx >> 6)) * gp + (tx0 >> 2) + ((tid & 15) >> 2)] = cmin;
                }
            }
        }
    }
    DBG_CLOCK(53, dbg);
    if (mode == 0 && minmax) {
        lmin = wave64_min(lmin); lmax = wave64_max(lmax);       // (a ds_bpermute butterfly here was ~1 us of the tile's ~4.5)
        if (tid == 0) {                                // reduced by k_blur_check_redo
            lv.tilemin[((size_t)p * lv.tmax + tby) * lv.tmax + tbx] = lmin;
            lv.tilemax[((size_t)p * lv.tmax + tby) * lv.tmax + tbx] = lmax;
        }
    }
    __syncthreads();                                   // LDS is reused by the block's next tile
    DBG_CLOCK(54, dbg);
}

// A free tile is the free-space constant: one wave, 64 lanes x 16 bytes = the tile's 256 cells (the whole tile, also beyond
// the current frame, so that the tile stays valid when the frame grows by its +-1 jitter), and its 4 x 4 block minima.
__device__ __forceinline__ uint32_t fill_value(const Slam2dLevel& lv) {
    const double v = lv.floor_value;
    return v > 0.5 * v ? 0u : (uint32_t)rint(-v * lv.cost_scale);
}
__device__ __forceinline__ void fill_tile(const Slam2dLevel& lv, int p, int t, int lane, const uint32_t c) {
    uint32_t* field = lv.field + (size_t)p * lv.fmax * lv.fpitch;
    const int ty0 = (t / lv.tmax) * BLUR_TILE, tx0 = (t % lv.tmax) * BLUR_TILE;
    const int y = lane >> 2, x = (lane & 3) * 4;
    if (ty0 + y < lv.fmax && tx0 + x + 3 < lv.fpitch)
        *reinterpret_cast<uint4*>(field + (size_t)(ty0 + y) * lv.fpitch + tx0 + x) = make_uint4(c, c, c, c);
    if (lv.bnb && lane < 16) {                             // the tile's 4 x 4 block minima (branch and bound)
        const int gp = lv.tmax << 2;
        lv.gmin[((size_t)p * gp + (ty0 >> 2) + (lane >> 2)) * gp + (tx0 >> 2) + (lane & 3)] = c;
    }
}

// Tile triage, one 1024-thread block per particle looping over its 16x16 field tiles:
//  * tiles with an occupied cell inside their blur halo -- an occupied 8x8-cell block (level->tilemask) within
//    ceil(radius / 8) blocks of the tile's four -- go to the blur work list;
//  * free tiles whose part of the field buffer does not already hold the free-space constant (tilestate) are
//    filled with it by this same block (no separate launch).
// lazy != 0 (slam2d_match): only tiles the sweep will read (lv.tileneed, marked by k_endpoints) are
// blurred or filled; the others keep their stale content and their tilestate.  This needs the field
// minimum (:43) to be known without computing the whole field: it is the analytic floor as soon as
// ONE tile of the frame is free (every cell of such a tile equals the floor and no blurred value is
// below it).  A frame without any free tile falls back to the full build.
#define TRIAGE_THREADS 1024
__global__ __launch_bounds__(TRIAGE_THREADS) void k_tile_triage(Slam2dLevel lv, int lazy) {
    // tile flags, tile states and the needed-tile bitmap of the particle are staged in LDS with one batch
    // of coalesced loads; everything after that runs out of LDS (the kernel is pure latency otherwise)
    extern __shared__ __attribute__((aligned(16))) uint8_t tri_lds[];     // block flag bits, [ntile4] states, [nneed] words, [ntile] fill list
    __shared__ int base[2];
    const int p = blockIdx.x, tid = threadIdx.x;
    const int lane = tid & 63, wave = tid >> 6;
    DBG_CLOCK(20, p == 0);
    const Slam2dFrame fr = lv.frames[p];
    const int nty = (fr.fh + BLUR_TILE - 1) >> BLUR_SHIFT, ntx = (fr.fw + BLUR_TILE - 1) >> BLUR_SHIFT;
    const int ntile = lv.tmax * lv.tmax, ntile4 = (ntile + 3) & ~3, nneed = (ntile + 31) >> 5;
    const int iters = (ntile + TRIAGE_THREADS - 1) / TRIAGE_THREADS;          // <= 32 (checked by the host)
    // the block flags as BITS in LDS -- one 16-bit word per 16-byte load, rows of `rw` words with a zero word in front, kb zero
    // rows above and below -- and, per tile row, the OR of the 2 + 2 kb flag rows its halo spans: a tile's test is one shift of
    // two words of its row (byte flags and a 4 x 4 window of LDS reads per tile cost three times the kernel's compute)
    const int kb = (lv.blur_radius + 7) >> FLAG_SHIFT;     // blocks the blur radius reaches beyond a tile (<= 2)
    const int fp = flag_pitch(lv), frows = lv.tmax << 1;
    const int rw = (fp >> 4) + 1, rw1 = rw + 1;
    uint16_t* bits_s = reinterpret_cast<uint16_t*>(tri_lds);                     // [kb + frows + kb][rw]
    uint16_t* rows_s = bits_s + (((frows + 2 * kb) * rw + 1) & ~1);              // [tmax][rw + 1] (a zero word at the end)
    const int fbytes = (2 * ((((frows + 2 * kb) * rw + 1) & ~1) + lv.tmax * rw1) + 15) & ~15;
    uint8_t* state_s = tri_lds + fbytes;
    uint32_t* need_s = reinterpret_cast<uint32_t*>(tri_lds + fbytes + ntile4);
    uint16_t* fill_s = reinterpret_cast<uint16_t*>(need_s + nneed);             // [ntile] the fill list
    const uint8_t stamp = occ_stamp(lv);
    uint8_t* state = lv.tilestate + (size_t)p * ntile;
    // every global load of the kernel's first half is issued before the first barrier -- flags, states AND the first words of
    // the needed-tile slices: the kernel is a chain of round trips, this makes it one instead of two
    constexpr int PRE = 4;
    const uint32_t* __restrict__ sl = need_slice(lv, p, 0, nneed);
    const int nsl = lazy ? nneed * need_slices(lv) : 0;
    uint32_t pre[PRE];
#pragma unroll
    for (int u = 0; u < PRE; ++u) { const int i = tid + u * TRIAGE_THREADS; pre[u] = i < nsl ? sl[i] : 0u; }
    {
        const uint4* tq = reinterpret_cast<const uint4*>(lv.tilemask + (size_t)p * flag_bytes(lv));     // (rows of fp bytes, fp % 16 == 0)
        const int qpr = fp >> 4, nq = frows * qpr;
        for (int i = tid; i < nq; i += TRIAGE_THREADS) {
            const uint4 v = tq[i];
            // bytes 0 / 1 -> one bit each: the multiplier moves byte k's bit 0 to bit 24 + k (no two partial products meet)
            const uint32_t m = ((bytes_equal(v.x, stamp) * 0x01020408u) >> 24) | (((bytes_equal(v.y, stamp) * 0x01020408u) >> 24) << 4) |
                               (((bytes_equal(v.z, stamp) * 0x01020408u) >> 24) << 8) | (((bytes_equal(v.w, stamp) * 0x01020408u) >> 24) << 12);
            const int row = i / qpr;
            bits_s[(kb + row) * rw + 1 + (i - row * qpr)] = (uint16_t)m;
        }
        for (int i = tid; i < frows; i += TRIAGE_THREADS) bits_s[(kb + i) * rw] = 0;
        for (int i = tid; i < kb * rw; i += TRIAGE_THREADS) { bits_s[i] = 0; bits_s[(kb + frows) * rw + i] = 0; }
        for (int t = tid; t < ntile; t += TRIAGE_THREADS) state_s[t] = state[t];
        if (lazy) for (int w = tid; w < nneed; w += TRIAGE_THREADS) need_s[w] = 0u;
    }
    if (tid < 2) base[tid] = 0;
    DBG_CLOCK(21, p == 0);
    __syncthreads();
    DBG_CLOCK(22, p == 0);
    if (lazy) {                                            // the particle's needed tiles: OR over the theta slices
#pragma unroll
        for (int u = 0; u < PRE; ++u)
            if (pre[u]) { const int w = (tid + u * TRIAGE_THREADS) % nneed; if ((need_s[w] & pre[u]) != pre[u]) atomicOr(&need_s[w], pre[u]); }
        for (int i = tid + PRE * TRIAGE_THREADS; i < nsl; i += TRIAGE_THREADS) {
            const uint32_t v = sl[i];
            if (v) { const int w = i % nneed; if ((need_s[w] & v) != v) atomicOr(&need_s[w], v); }
        }
    }
    for (int i = tid; i < lv.tmax * rw1; i += TRIAGE_THREADS) {                // the flag rows of a tile row's halo, ORed
        const int ty = i / rw1, j = i - ty * rw1;
        uint32_t v = 0u;
        if (j < rw) for (int k = 0; k < 2 + 2 * kb; ++k) v |= bits_s[(2 * ty + k) * rw + j];
        rows_s[i] = (uint16_t)v;
    }
    __syncthreads();
    DBG_CLOCK(23, p == 0);
    uint32_t liveb = 0u, anyb = 0u;
    int has_free = 0;
    for (int it = 0; it < iters; ++it) {
        const int t = it * TRIAGE_THREADS + tid;
        const int ty = t / lv.tmax, tx = t - ty * lv.tmax;
        if (t < ntile && ty < nty && tx < ntx) {
            // a wall within the blur radius of the tile <=> an occupied 8 x 8 block within kb blocks of the tile's four (flags
            // beyond the frame and the border read 0)
            // flag columns 2 tx - kb .. 2 tx + 1 + kb of the tile row's OR (bit 16 of the row = flag column 0)
            const int bit = 2 * tx - kb + 16;
            const uint16_t* r16 = rows_s + ty * rw1 + (bit >> 4);
            const int any = (((uint32_t)r16[0] | ((uint32_t)r16[1] << 16)) >> (bit & 15)) & ((1u << (2 + 2 * kb)) - 1u);
            liveb |= 1u << it;
            if (any) anyb |= 1u << it; else has_free = 1;
        }
    }
    DBG_CLOCK(24, p == 0);
    has_free = __syncthreads_or(has_free);
    DBG_CLOCK(25, p == 0);
    // one free tile pins the field minimum (:43) to the analytic floor: k_blur_check_redo has nothing to do
    if (tid == 0) lv.frames[p].min_known = has_free;
    const bool everything = !lazy || !has_free;
    int* list = lv.tilelist + (size_t)p * 2 * ntile;
    // list positions from LDS counters (one aggregated atomic per wave and list): the order of a list does not
    // matter -- every tile is blurred / filled independently -- and the loop needs no barrier
    const unsigned long long below = lane ? (~0ull >> (64 - lane)) : 0ull;
    for (int it = 0; it < iters; ++it) {
        const int t = it * TRIAGE_THREADS + tid;
        const bool live = (liveb >> it) & 1u, any = (anyb >> it) & 1u;
        const bool wanted = live && (everything || ((need_s[t >> 5] >> (t & 31)) & 1u));
        bool to_fill = false;
        // (a free tile's minimum is the floor -- not recorded: k_blur_check_redo reads the per-tile minima only when the frame
        // has no free tile at all, and then every tile goes through the blur, which records its own)
        if (live && !any && wanted && state_s[t] != 0) { to_fill = true; state[t] = 0; }
        const bool mine[2] = {wanted && any, to_fill};
#pragma unroll
        for (int which = 0; which < 2; ++which) {
            const unsigned long long mask = __ballot(mine[which]);
            if (!mask) continue;
            int start = 0;
            if (lane == 0) start = atomicAdd(&base[which], __popcll(mask));
            start = __builtin_amdgcn_readfirstlane(start);
            if (mine[which]) {
                list[which * ntile + start + __popcll(mask & below)] = t;
                if (which) fill_s[start + __popcll(mask & below)] = (uint16_t)t;           // (t < 32 * 1024)
            }
        }
    }
    DBG_CLOCK(26, p == 0);
    __syncthreads();
    if (tid < 2) lv.tilecount[2 * p + tid] = base[tid];
    DBG_CLOCK(27, p == 0);
    // fill: one wave per tile, the tiles from the LDS copy of the list
    const int nfill = base[1];
    const uint32_t c = fill_value(lv);
    for (int b = wave; b < nfill; b += TRIAGE_THREADS / 64) fill_tile(lv, p, fill_s[b], lane, c);
}

// Blur of the work list: bpp one-wave blocks per particle walk that particle's active tiles.
#ifndef BLUR_MIN_WAVES
#define BLUR_MIN_WAVES 1
#endif
// The grid is 1-D (round 4): block b runs on XCD b % 8 and all blocks of particle p on XCD p % 8, like the sweep's
// and the update's -- x-adjacent tiles share the 128-byte lines of their occupancy halo (8 tiles wide), and with the blocks of a
// particle dealt round the XCDs by blockIdx.x every XCD's L2 fetched its own copy of those lines (round 3: 34 MB of HBM
// traffic per 32-particle launch for 6.9 MB processed, L2 hit rate 56 % with the (blocks, P) grid of rounds 1-3).
// tail != 0 (levels where k_blur_check_redo is not launched, fold_field_check: those without bounds since round 4, and those whose
// bounds k_bound_lds takes -- blur_tile's redo rewrites the block minima gmin, that kernel derives gmin2 from them): the minimum check of a frame
// WITHOUT a free tile -- rare: then every tile was listed and blurred against the analytic floor -- is done by the last of the
// particle's blur blocks to finish (arrival counter lv.sync[p][1]; plain stores + agent release before the ticket, agent acquire
// after it: the slow, always-valid form -- it runs once in a blue moon).  A frame with a free tile, the normal case, costs nothing.
template <int RAD>
__device__ __forceinline__ void blur_check_tail(const Slam2dLevel& lv, BlurLds<RAD>& sm, const int p, Slam2dFrame fr, uint32_t* flags) {
    const int tid = threadIdx.x;
    const int nty = (fr.fh + BLUR_TILE - 1) >> BLUR_SHIFT, ntx = (fr.fw + BLUR_TILE - 1) >> BLUR_SHIFT;
    const double* __restrict__ tm = lv.tilemin + (size_t)p * lv.tmax * lv.tmax;
    double m = INFINITY;
    for (int t = tid; t < nty * ntx; t += BLUR_THREADS) m = fmin(m, tm[(t / ntx) * lv.tmax + (t % ntx)]);
    m = wave64_min(m);
    if (tid == 0) {
        lv.frames[p].field_min = m;
        if (m != lv.floor_value) { lv.frames[p].redo = 1; atomicOr(&flags[p], SLAM2D_F_FLOOR_REDO); }
    }
    if (m == lv.floor_value) return;                   // (wave-uniform)
    fr.field_min = m;
    for (int t = 0; t < nty * ntx; ++t) blur_tile<RAD>(lv, sm, p, fr, t / ntx, t % ntx, 1, true);
}
template <int RAD>
__global__ __launch_bounds__(BLUR_THREADS, RAD == 8 ? 4 : BLUR_MIN_WAVES) void k_blur_clamp(Slam2dLevel lv, int P, int bpp, uint32_t* flags, int tail) {
    __shared__ BlurLds<RAD> sm;
    const int xcd = blockIdx.x & 7, slot = blockIdx.x >> 3;
    const int p = (slot / bpp) * 8 + xcd, first = slot % bpp;
    if (p >= P) return;
    // the block's first list entry and the frame are requested with the count, not behind it (each a round trip to what the
    // triage has just written); the entry may be a stale one (first >= n: slot `first` clamped into the particle's lists) and
    // is used only when it is not.  What the tiles need of the frame: its size and min_known.  (The empty asm is the values'
    // first use: without it the compiler sinks the loads behind the count's branch.)
    const int* list = lv.tilelist + (size_t)p * 2 * lv.tmax * lv.tmax;
    int t0 = list[min(first, 2 * lv.tmax * lv.tmax - 1)];
    Slam2dFrame fr = lv.frames[p];
    int n = lv.tilecount[2 * p];
    asm volatile("" : "+s"(t0), "+s"(fr.fh), "+s"(fr.fw), "+s"(fr.min_known), "+s"(n));      // (all four arrive with one wait)
    if (first >= n) return;
    // the per-tile minima and maxima have two readers: blur_check_tail below (a frame without a free tile) and k_blur_check_redo,
    // which is not launched where tail != 0
    const bool minmax = !(tail && fr.min_known);
    for (int b = first; b < n; b += bpp) {
        const int t = b == first ? t0 : list[b];
        blur_tile<RAD>(lv, sm, p, fr, t / lv.tmax, t % lv.tmax, 0, false, minmax);
    }
    if (tail && !fr.min_known) {                       // (block-uniform; rare)
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");                       // this wave's per-tile minima leave the XCD's L2
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        unsigned ticket = 0u;
        if (threadIdx.x == 0) ticket = __hip_atomic_fetch_add(&lv.sync[p * SLAM2D_SYNC_WORDS + 1], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        ticket = (unsigned)__builtin_amdgcn_readfirstlane((int)ticket);
        if (ticket != (unsigned)(min(n, bpp) - 1)) return;                   // (blocks of this particle that had a tile)
        if (threadIdx.x == 0) __hip_atomic_store(&lv.sync[p * SLAM2D_SYNC_WORDS + 1], 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
        blur_check_tail<RAD>(lv, sm, p, fr, flags);
    }
}

#ifndef GMIN2_ROWWISE
#define GMIN2_ROWWISE 1
#endif
#define GMIN2_BLOCKS 16              // blocks per particle of k_blur_check_redo where it derives gmin2
// gmin2 (branch and bound): element [Y][X] = min(gmin[Y..Y+1][X..X+1]) >> 12.  Blocks beyond the buffer are clamped
// (duplicates only).
// The arithmetic of an entry, shared by k_blur_check_redo (gmin2_entry, gmin2_dirty) and by k_bound_lds's prologue (bound_refresh_*): both
// must leave the same bits in memory.
typedef unsigned int gu4 __attribute__((ext_vector_type(4)));
// one entry: the minimum of its 2 x 2 block minima (indices clamped to the image)
__device__ __forceinline__ uint32_t gmin2_min2x2(const uint32_t* __restrict__ G, const int gp, const int Y, const int X) {
    const int Y1 = min(Y + 1, gp - 1), X1 = min(X + 1, gp - 1);
    return min(min(G[(size_t)Y * gp + X], G[(size_t)Y * gp + X1]), min(G[(size_t)Y1 * gp + X], G[(size_t)Y1 * gp + X1]));
}
// the 5 entries X = 4 tx - 1 .. 4 tx + 3 of row Y of a tile's reach: `em` and e.x .. e.w, unshifted.  Row-wise only for a tile off
// the image's border (gmin2_row_on_border: those go entry by entry): two block-minima rows as 1 + 4 + 1 values each, the
// middle four one aligned 16-byte load.
struct Gmin2Row { uint32_t em; gu4 e; };
__device__ __forceinline__ bool gmin2_row_on_border(const int tmax, const int gp, const int tx, const int Y) {
    return tx == 0 || tx >= tmax - 1 || Y + 1 >= gp;
}
__device__ __forceinline__ Gmin2Row gmin2_row_minima(const uint32_t* __restrict__ G, const int gp, const int Y, const int tx) {
    const uint32_t* __restrict__ r0 = G + (size_t)Y * gp + 4 * tx;
    const uint32_t* __restrict__ r1 = r0 + gp;
    const uint32_t am = r0[-1], ap = r0[4], bm = r1[-1], bp = r1[4];
    const gu4 a = *reinterpret_cast<const gu4*>(r0), b = *reinterpret_cast<const gu4*>(r1);
    const uint32_t cm = min(am, bm), c0 = min(a.x, b.x), c1 = min(a.y, b.y), c2 = min(a.z, b.z), c3 = min(a.w, b.w), cp = min(ap, bp);
    Gmin2Row row;
    row.em = min(cm, c0);
    row.e.x = min(c0, c1); row.e.y = min(c1, c2); row.e.z = min(c2, c3); row.e.w = min(c3, cp);
    return row;
}
// what is stored of a row: gmin2 holds >> 12 (o = the entry at X = 4 tx), the byte image >> 24 (ob likewise, an aligned word)
__device__ __forceinline__ uint32_t gmin2_row_bytes(const Gmin2Row& row) {
    return (row.e.x >> 24) | ((row.e.y >> 24) << 8) | ((row.e.z >> 24) << 16) | ((row.e.w >> 24) << 24);
}
__device__ __forceinline__ void gmin2_row_store_words(const Gmin2Row& row, uint32_t* __restrict__ o) {
    o[-1] = row.em >> 12;
    gu4 ov; ov.x = row.e.x >> 12; ov.y = row.e.y >> 12; ov.z = row.e.z >> 12; ov.w = row.e.w >> 12;
    *reinterpret_cast<gu4*>(o) = ov;
}
template <typename B>
__device__ __forceinline__ void gmin2_row_store_bytes(const Gmin2Row& row, B* ob) {
    ob[-1] = (B)(row.em >> 24);
    *reinterpret_cast<uint32_t*>(ob) = gmin2_row_bytes(row);
}
__device__ __forceinline__ void gmin2_entry(const Slam2dLevel& lv, const uint32_t* __restrict__ G, uint32_t* __restrict__ G2,
                                            const int p, const int gp, const int Y, const int X) {
    const int Y1 = min(Y + 1, gp - 1), X1 = min(X + 1, gp - 1);
    const uint32_t v = gmin2_min2x2(G, gp, Y, X);
    G2[(size_t)Y * gp + X] = v >> 12;
    if (lv.gmin2b) lv.gmin2b[((size_t)p * gp + Y) * lv.g2b_pitch + X] = (uint8_t)(v >> 24);      // (k_bound_lds)
    if (lv.bnb == 2) {
        // two-level bounds: the 8x8 cell window of an 8x8-pose tile lies inside blocks Y..Y+2 x X..X+2; stored decimated by
        // two in four phase planes, so that the tiles of one row (block stride 2) are contiguous
        const int Y2 = min(Y + 2, gp - 1), X2 = min(X + 2, gp - 1);
        uint32_t v3 = min(v, min(G[(size_t)Y * gp + X2], G[(size_t)Y1 * gp + X2]));
        v3 = min(v3, min(min(G[(size_t)Y2 * gp + X], G[(size_t)Y2 * gp + X1]), G[(size_t)Y2 * gp + X2]));
        const int hp = gp >> 1;
        lv.gmin3d[(size_t)p * gp * gp + ((size_t)(((Y & 1) << 1) | (X & 1)) * hp + (Y >> 1)) * hp + (X >> 1)] = v3 >> 12;
    }
}
// ... over the whole frame: `part` of `parts` thread groups of `nthreads` threads each
__device__ __forceinline__ void gmin2_pass(const Slam2dLevel& lv, const int p, const Slam2dFrame& fr, const int tid,
                                           const int nthreads, const int part, const int parts) {
    const int gp = lv.tmax << 2;
    const int rows = min(gp, (fr.fh >> 2) + 2), cols = min(gp, (fr.fw >> 2) + 2);
    const uint32_t* __restrict__ G = lv.gmin + (size_t)p * gp * gp;
    uint32_t* __restrict__ G2 = lv.gmin2 + (size_t)p * gp * gp;
    for (int idx = part * nthreads + tid; idx < rows * cols; idx += parts * nthreads) {
        const int Y = idx / cols, X = idx - Y * cols;
        gmin2_entry(lv, G, G2, p, gp, Y, X);
    }
}
// ... over the entries that can have changed: a tile written at this build (the blur list and the fill list of the triage)
// changes the minima of its own 4 x 4 blocks, hence entries Y in [4 ty - 1, 4 ty + 3] (from 4 ty - 2 with gmin3d), likewise
// X.  An entry the bounds read covers cells of tiles that are all needed, hence current: either rebuilt now (listed) or
// holding the free-space constant since they were last written -- and every write of a tile has refreshed all the entries it
// touches, so the entry equals what the whole-frame pass would store.  (That pass read and wrote 2 x 166 KB per particle
// and scan for ~150 changed tiles: 21.7 MB of HBM traffic per launch at config 2.)
__device__ __forceinline__ void gmin2_dirty(const Slam2dLevel& lv, const int p, const int tid, const int nthreads,
                                            const int part, const int parts) {
    const int gp = lv.tmax << 2, ntile = lv.tmax * lv.tmax;
    const int nb = lv.tilecount[2 * p], nf = lv.tilecount[2 * p + 1];
    const int* __restrict__ list = lv.tilelist + (size_t)p * 2 * ntile;
    const int E = lv.bnb == 2 ? 6 : 5, per = E * E;
    const uint32_t* __restrict__ G = lv.gmin + (size_t)p * gp * gp;
    uint32_t* __restrict__ G2 = lv.gmin2 + (size_t)p * gp * gp;
    if (lv.bnb != 2 && GMIN2_ROWWISE) {
        // 5 x 5 entries per tile, one thread per (tile, entry row): the two block-minima rows it needs as 1 + 4 + 1 values each (the
        // middle four are one aligned 16-byte load), five entries out as 1 + 4 -- 6 loads and 2 (+ 2 byte-image) stores per row where
        // the entry-per-thread form below issued 20 and 5 (+ 5); same minima, same bits.  Tiles on the image's border go entry by entry.
        for (int idx = part * nthreads + tid; idx < (nb + nf) * 5; idx += parts * nthreads) {
            const int k = idx / 5, r = idx - k * 5;
            const int t = k < nb ? list[k] : list[ntile + (k - nb)];
            const int ty = t / lv.tmax, tx = t - ty * lv.tmax;
            const int Y = 4 * ty - 1 + r;
            if (Y < 0 || Y >= gp) continue;
            if (gmin2_row_on_border(lv.tmax, gp, tx, Y)) {
                for (int c = 0; c < 5; ++c) {
                    const int X = 4 * tx - 1 + c;
                    if (X >= 0 && X < gp) gmin2_entry(lv, G, G2, p, gp, Y, X);
                }
                continue;
            }
            const Gmin2Row row = gmin2_row_minima(G, gp, Y, tx);
            gmin2_row_store_words(row, G2 + (size_t)Y * gp + 4 * tx);
            if (lv.gmin2b) gmin2_row_store_bytes(row, lv.gmin2b + ((size_t)p * gp + Y) * lv.g2b_pitch + 4 * tx);
        }
        return;
    }
    for (int idx = part * nthreads + tid; idx < (nb + nf) * per; idx += parts * nthreads) {
        const int k = idx / per, e = idx - k * per;
        const int t = k < nb ? list[k] : list[ntile + (k - nb)];
        const int ty = t / lv.tmax, tx = t - ty * lv.tmax;
        const int Y = 4 * ty - (E - 4) + e / E, X = 4 * tx - (E - 4) + e % E;
        if (Y < 0 || X < 0 || Y >= gp || X >= gp) continue;
        gmin2_entry(lv, G, G2, p, gp, Y, X);
    }
}

// probMin (:43) = minimum over the per-tile minima; when it is not the analytic floor (rare: no cell
// of the field has an all-free neighbourhood) the clamp is redone with it.  Block (p, 0) does that; with branch
// and bound, blocks (p, 0 .. gridDim.y-1) also derive gmin2 from the block minima the blur just wrote -- all of them
// at once when a free tile pins the minimum (frames[p].min_known, set by the triage: no redo can follow), block
// (p, 0) alone after the check otherwise.
template <int RAD>
__global__ __launch_bounds__(256) void k_blur_check_redo(Slam2dLevel lv, uint32_t* flags, int dirty_only) {
    __shared__ BlurLds<RAD> sm;
    __shared__ double red_s[4];
    const int p = blockIdx.x, tid = threadIdx.x;
    Slam2dFrame fr = lv.frames[p];
    if (lv.bnb && fr.min_known) {
        if (dirty_only) gmin2_dirty(lv, p, tid, 256, blockIdx.y, gridDim.y);
        else gmin2_pass(lv, p, fr, tid, 256, blockIdx.y, gridDim.y);
    }
    if (blockIdx.y != 0) return;
    {   // largest value any pose can read: free tiles hold the floor, the blurred ones recorded theirs
        const int n = lv.tilecount[2 * p];
        const int* list = lv.tilelist + (size_t)p * 2 * lv.tmax * lv.tmax;
        double mx = lv.floor_value > 0.5 * lv.floor_value ? 0.0 : lv.floor_value;
        for (int i = tid; i < n; i += 256) mx = fmax(mx, lv.tilemax[(size_t)p * lv.tmax * lv.tmax + list[i]]);
        mx = wave64_max(mx);
        if ((tid & 63) == 0) red_s[tid >> 6] = mx;
        __syncthreads();
        if (tid == 0) lv.frames[p].field_max = fmax(fmax(red_s[0], red_s[1]), fmax(red_s[2], red_s[3]));
        __syncthreads();
    }
    // bit tx of freerow[ty]: tile (ty, tx) of the field buffer holds the free-space constant (k_sweep skips
    // loads whose whole patch lies in such tiles)
    if (sweep_skips(lv) && tid < 64) {
        unsigned long long bits = 0ull;
        if (tid < lv.tmax) {
            const uint8_t* st = lv.tilestate + ((size_t)p * lv.tmax + tid) * lv.tmax;
            for (int tx = 0; tx < lv.tmax; ++tx) bits |= (unsigned long long)(st[tx] == 0) << tx;
        }
        lv.freerow[(size_t)p * 64 + tid] = fr.min_known ? bits : 0ull;       // not when the clamp may be redone
    }
    if (fr.min_known) return;                          // a free tile exists: the minimum is the analytic floor
    const int nty = (fr.fh + BLUR_TILE - 1) >> BLUR_SHIFT, ntx = (fr.fw + BLUR_TILE - 1) >> BLUR_SHIFT;
    const double* __restrict__ tm = lv.tilemin + (size_t)p * lv.tmax * lv.tmax;
    double m = INFINITY;
    for (int t = tid; t < nty * ntx; t += 256) m = fmin(m, tm[(t / ntx) * lv.tmax + (t % ntx)]);
    m = wave64_min(m);
    if ((tid & 63) == 0) red_s[tid >> 6] = m;
    __syncthreads();
    m = fmin(fmin(red_s[0], red_s[1]), fmin(red_s[2], red_s[3]));
    if (tid == 0) {
        lv.frames[p].field_min = m;
        if (m != lv.floor_value) { lv.frames[p].redo = 1; atomicOr(&flags[p], SLAM2D_F_FLOOR_REDO); }
    }
    if (m == lv.floor_value) {                         // (block-uniform)
        if (lv.bnb) gmin2_pass(lv, p, fr, tid, 256, 0, 1);
        return;
    }
    if (tid >= BLUR_THREADS) return;                   // the redo itself is one wave's work
    fr.field_min = m;
    for (int t = 0; t < nty * ntx; ++t) blur_tile<RAD>(lv, sm, p, fr, t / ntx, t % ntx, 1, true);
    if (lv.bnb) gmin2_pass(lv, p, fr, tid, BLUR_THREADS, 0, 1);
}

// ------------------------------------------------------------------------------------
// K1b  motion priors rv / thetaWeight              (Utils/ScanMatcher_OGBased.py:97-110)
//      prior[p][0] = rv, prior[p][1] = thetaWeight, each [ny][nx]; computed by the extra block of
//      k_endpoints' extra block of the particle
// ------------------------------------------------------------------------------------
// Pruning by the motion prior (slam2d_match with SLAM2D_MATCH_PRUNE_BY_PRIOR, coarse level only).
// The reference forces rv = -100 wherever the pose's distance from the estimate differs from the
// odometry step by more than maxMoveDeviation (:102-103); field sums and thetaWeight are <= 0, so every
// pose outside that ring scores <= -100.  The sweep first scores the ring alone (a few per cent of the
// cube); if the best ring pose beats -100 + K * (largest value of the field) by SLAM2D_PRUNE_MARGIN = 40, no
// pose outside the ring can be the arg-max and all of them together add less than 1e-12 (relative) to the
// confidence and to the soft-max draw.  Otherwise -- or when a pose outside the ring has a NaN prior, which the reference's argmax would
// return -- the particle is swept in full by a second, normally empty, launch.
// prune_ring(): is pose offset (xv, yv) inside the ring?  The very expression that decides rv below.
__device__ __forceinline__ bool prune_ring(const Slam2dLevel& lv, const int xv, const int yv, const double est_dist) {
    const double mx = (double)xv * lv.step, my = (double)yv * lv.step;
    return !(fabs(sqrt(mx * mx + my * my) - est_dist) > lv.max_move_dev);
}

__device__ __forceinline__ void write_priors(const Slam2dLevel& lv, const int p, const double est_dist,
                                             const double* __restrict__ psi_cs, const int prune) {
    __shared__ int ring_cnt[4];
    __shared__ int ring_base;
    const Cube cube = cube_of(lv);
    const int nx = cube.nx, np_ = cube.npose;
    double* out = lv.prior + (size_t)p * 2 * np_;
    const double cpsi = psi_cs ? psi_cs[2 * p] : NAN;
    const double spsi = psi_cs ? psi_cs[2 * p + 1] : NAN;
    int need_full = 0;
    for (int q = threadIdx.x; q < np_; q += blockDim.x) {
        double rv = 0.0, tw = 0.0;
        if (!lv.fine) {
            const int iy = q / nx, ix = q - iy * nx;
            const int xv = ix - lv.ncell, yv = iy - lv.ncell;
            const double mx = (double)xv * lv.step, my = (double)yv * lv.step;
            const double dist = sqrt(mx * mx + my * my);
            const double dev = dist - est_dist;
            rv = lv.rv_coef * (dev * dev);                                          // :101
            if (fabs(dev) > lv.max_move_dev) rv = -100.0;                           // :102-103
            if (!isnan(cpsi)) {                                                     // :104-108
                double dv = sqrt((double)(xv * xv + yv * yv));
                if (dv == 0.0) dv = 0.0001;
                const double arg = ((double)xv * cpsi + (double)yv * spsi) / dv;
                const double th = acos(arg);            // NaN when |arg| > 1, as np.arccos
                tw = lv.tw_coef * (th * th);
            }
            if (prune && isnan(tw) && !prune_ring(lv, xv, yv, est_dist)) need_full = 1;
        }
        out[q] = rv;
        out[np_ + q] = tw;
    }
    if (lv.bnb && lv.bnb != 3) {
        // largest rv + thetaWeight of every 4x4 pose tile (+inf when one of them is NaN: np.argmax returns the first
        // NaN, so such a tile is always scored); padding tiles get -inf
        __syncthreads();                                   // the planes above were written by this block
        const int nbt = cube.nbt, nbq4 = cube.nbq4;
        double* pm = lv.tile_pmax + (size_t)p * nbt * nbq4;
        for (int t = threadIdx.x; t < nbt * nbq4; t += blockDim.x) {
            const int by = t / nbq4, bx = t - by * nbq4;
            double m = -INFINITY;
            if (bx < nbt)
                for (int r = 0; r < 4 && 4 * by + r < nx; ++r)
                    for (int e = 0; e < 4 && 4 * bx + e < nx; ++e) {
                        const int q = (4 * by + r) * nx + 4 * bx + e;
                        const double v = out[q] + out[np_ + q];
                        m = isnan(v) ? INFINITY : fmax(m, v);
                    }
            pm[t] = m;
        }
    }
    if (!prune) return;
    need_full = __syncthreads_or(need_full);
    if (threadIdx.x == 0) lv.prune_state[p] = need_full;
    if (p != 0) return;
    // the ring as an ascending list of sweep slots (4 consecutive dx of one dy), shared by all particles
    const int nslot = cube.nslot;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (threadIdx.x == 0) ring_base = 0;
    __syncthreads();
    for (int s0 = 0; s0 < nslot; s0 += (int)blockDim.x) {
        const int u = s0 + threadIdx.x;
        bool in = false;
        if (u < nslot) {
            const int iy = u / cube.nq, dx = (u - iy * cube.nq) * 4;
            for (int e = 0; e < 4 && dx + e < nx; ++e) in = in || prune_ring(lv, dx + e - lv.ncell, iy - lv.ncell, est_dist);
        }
        const unsigned long long mask = __ballot(in);
        if (lane == 0) ring_cnt[wave] = __popcll(mask);
        __syncthreads();
        int pos = ring_base + __popcll(mask & (lane ? (~0ull >> (64 - lane)) : 0ull));
        for (int w2 = 0; w2 < wave; ++w2) pos += ring_cnt[w2];
        if (in && pos < lv.ring_cap) lv.ring[1 + pos] = u;
        __syncthreads();
        if (threadIdx.x == 0) for (int w2 = 0; w2 < (int)(blockDim.x >> 6); ++w2) ring_base += ring_cnt[w2];
        __syncthreads();
    }
    if (threadIdx.x == 0) lv.ring[0] = ring_base <= lv.ring_cap ? ring_base : -1;     // -1: does not fit, sweep in full
}

// k_frame_axis's per-particle work, done by one 256-thread block (the priors block of k_endpoints) when that
// kernel is not launched: frame, flags, axis tables (:21-37,173-176).
__device__ __forceinline__ void frame_duties(const Slam2dLidar& lid, const Slam2dLevel& lv, const Slam2dMap* __restrict__ maps,
                                             const double* __restrict__ centre, const int cstride, uint32_t* flags, const int p) {
    const Slam2dMap m = maps[p];
    uint32_t f;
    const Slam2dFrame fr = make_frame(lid, lv, m, centre[(size_t)p * cstride], centre[(size_t)p * cstride + 1], f);
    if (threadIdx.x == 0) frame_publish(lv, p, fr, f, flags);
    bool bad = false;
    for (int axis = 0; axis < 2; ++axis)
        for (int j = threadIdx.x; j < axis_length(fr, axis); j += blockDim.x) bad = !axis_table_store(lv, m, fr, p, axis, j) || bad;
    if (bad) atomicOr(&flags[p], SLAM2D_F_FIELD_INDEX);
}

// ------------------------------------------------------------------------------------
// K1a  beam endpoints -> unique field cells per theta   (Utils/ScanMatcher_OGBased.py:81-89,
//      117-121,162-176).  One block per (theta, particle); np.unique through an LDS hash set, ordered
//      compaction; plus one block per particle for the motion priors.
//      A cell is stored as the offset of the corner of its (2*ncell+1)^2 patch:
//      (cy - ncell) * fpitch + (cx - ncell).
// ------------------------------------------------------------------------------------
// NT threads: 256, or 192 for scans of up to 192 beams (one beam per thread; 10 blocks per CU instead of 8 hold all the
// 36 x 64 + 128 blocks of config 2 at once -- no second, nearly empty round)
template <int NT>
__global__ __launch_bounds__(NT) void k_endpoints(Slam2dLidar lid, Slam2dLevel lv, const double* __restrict__ est,
                                                   int estride, const double* __restrict__ ranges, uint32_t* flags,
                                                   double est_dist, const double* __restrict__ psi_cs, int mark, int prune,
                                                   int beam_table, const Slam2dMap* __restrict__ maps, int scatter_bx) {
    // maps != NULL: this launch is not preceded by k_frame_axis (slam2d_match below 512 beams): the theta blocks derive
    // the frame fields they need themselves, the priors block also writes frames[p], the axis tables and the flags.
    // np.unique (:120) through an LDS hash set: every beam inserts its cell; of the beams that hit one
    // cell the lowest beam index owns it (atomicMin), so the list keeps beam order -- which is spatially
    // coherent (neighbouring beams hit neighbouring cells) and deterministic.  Scores are exact
    // integer sums, so the order of the list cannot change a result.
    // mark != 0 (slam2d_match): the block also ORs the 16x16 field tiles its patches touch into
    // lv.tileneed (corner bits in LDS, dilated once per block), so that the field build can skip every other tile.
    extern __shared__ __attribute__((aligned(16))) int ep_lds[];     // [hsize] keys, [hsize] owners, [32] (step, wave) counts, tile-marking scratch
    // A block walks lv.ep_group adjacent angles one after the other: the beam endpoints (and, below 512 beams, their
    // cos / sin) are evaluated once per block, and the tile marks of all its angles are dilated and stored once.
    const int grp = blockIdx.x, p = blockIdx.y, tid = threadIdx.x;
    const int G = max(lv.ep_group, 1), ngrp = (lv.ntheta + G - 1) / G;
    if (grp == ngrp) {                                     // the extra block of every particle: motion priors (+ ring)
        write_priors(lv, p, est_dist, psi_cs, prune);
        return;
    }
    if (grp == ngrp + 1) {                                 // a second one (only when maps != NULL): what k_frame_axis would have done
        frame_duties(lid, lv, maps, est, estride, flags, p);
        return;
    }
    if (grp > ngrp + 1) {                                  // (scatter_bx > 0) the occupied-cell scatter, beside the angle blocks
        const int sb = grp - (ngrp + 2);
        scatter_role<NT / 64>(lid, lv, maps, est, estride, p, sb % scatter_bx, sb / scatter_bx, ep_lds);
        return;
    }
    const int it0 = grp * G, it1 = min(it0 + G, lv.ntheta);
    const double ex = est[(size_t)p * estride], ey = est[(size_t)p * estride + 1];
    Slam2dFrame fr;
    if (maps) {
        // no k_frame_axis ahead of this launch: the four frame fields used here (the frame block flags what is clamped)
        const FrameExtent e = frame_extent(lv, ex, ey);
        fr.xlo = e.xlo; fr.ylo = e.ylo;
        fr.fw = min(e.fw, lv.fmax); fr.fh = min(e.fh, lv.fmax);
    } else {
        fr = lv.frames[p];
    }
    const int B = lid.beams;
    DBG_CLOCK(40, grp == 0 && p == 0);
    constexpr int NW = NT / 64;
    const int hsize = endpoints_hash_size(B), hmask = hsize - 1;
    int* hkey = ep_lds;
    int* hown = ep_lds + hsize;
    int* cnt_s = ep_lds + 2 * hsize;
    for (int i = tid; i < hsize; i += NT) { hkey[i] = INT_MAX; hown[i] = INT_MAX; }
    // tile marking scratch: the patch of a beam covers tiles [tx0, tx0 + n + cx] x [ty0, ty0 + n + cy] with cx, cy in {0, 1}
    // (n = 2 ncell / 16), so a beam sets ONE bit -- its corner tile, in the bitmap of its class (cy, cx) -- and the
    // block dilates the four bitmaps afterwards (rows padded to whole words).  Walking the tile rows per beam was half of
    // this kernel's time at 1081 beams.
    const int nneed = (lv.tmax * lv.tmax + 31) >> 5;
    const int wp = (lv.tmax + 31) >> 5;                    // words per tile row
    uint32_t* corner_s = reinterpret_cast<uint32_t*>(ep_lds + 2 * hsize + 32);       // [2 cy][2 cx][tmax][wp]
    uint32_t* hd_s = corner_s + 4 * lv.tmax * wp;                                   // [2 cy][tmax][wp] after the horizontal pass
    uint32_t* lin_s = hd_s + 2 * lv.tmax * wp;                                      // [nneed] the block's bitmap (bit = ty * tmax + tx)
    uint32_t* const need_g = mark ? need_slice(lv, p, grp, nneed) : nullptr;
    if (mark) for (int i = tid; i < 6 * lv.tmax * wp + nneed; i += NT) corner_s[i] = 0u;   // (tmax^2 <= 28000, check_field_args: <= 28 KB)
    // Branch and bound: gmin2 summarises the aligned 8x8 blocks around the 4x4 windows of the pose tiles, which reach from 3 cells
    // before the patch to 4 * ceil(nx / 4) + 3 cells after its corner (two-level bounds: up to 8 * ceil(nx / 8) + 3).  Still only
    // the cells the POSES read are marked (round 4), (2 ncell + 1)^2 at the patch, as without bounds.  A block minimum taken
    // partly over cells of tiles that were not rebuilt is a minimum over MORE values than the poses can read: never larger than
    // the true one, so the bound it enters stays an upper bound of the scores -- only looser where a pose tile hangs over the
    // window's edge -- and whatever is scored exactly reads needed cells only.
    const int nc = lv.ncell;
    const int span = 2 * nc, ntl = span >> BLUR_SHIFT;
    const int per = NT == 256 ? (B + 255) / 256 : 1;       // beams per thread (5 at 1081 beams -- rounding the beams up to a power of
    //                                                        two first made it 8: three fully masked passes through every loop below,
    //                                                        a third of the kernel's vector instructions), interleaved: beam = q * NT + tid, so that a
    //                                                        wave's loads and stores are contiguous (at 1081 beams the
    //                                                        thread-contiguous mapping cost 32 cache lines per wave-load)
    const BeamFan fan = fan_of(lid, est[(size_t)p * estride + 2]);
    constexpr int QMAX = NT == 256 ? SLAM2D_MAX_BEAMS / 256 : 1;
    int key[QMAX], slot[QMAX];
    double bdx[QMAX], bdy[QMAX];                           // beam endpoint - estimate (:167-168), NaN: no return (:84)
    bool bad = false;
#pragma unroll
    for (int q = 0; q < QMAX; ++q) {
        bdx[q] = NAN; bdy[q] = NAN;
        const int b = q * NT + tid;
        if (q < per && b < B) {
            const double rg = ranges[b];
            if (rg < lid.max_range) {                                               // :84
                double px, py;
                if (beam_table) {                           // k_frame_axis evaluated :87-88 once for the particle
                    px = lv.beam_xy[((size_t)p * B + b) * 2]; py = lv.beam_xy[((size_t)p * B + b) * 2 + 1];
                } else {
                    const double a = fan.angle(b);
                    px = ex + cos(a) * rg; py = ey + sin(a) * rg;                   // :87-88
                }
                bdx[q] = px - ex; bdy[q] = py - ey;
            }
        }
    }
  for (int it = it0; it < it1; ++it) {                     // (indentation kept: the body is one angle's pass)
    const double c = lv.theta_cos[it], s = lv.theta_sin[it];
    if (it > it0) {                                        // the previous angle's compaction is past its barrier: the hash
        for (int i = tid; i < hsize; i += NT) { hkey[i] = INT_MAX; hown[i] = INT_MAX; }      // set is free again
    }
#pragma unroll
    for (int q = 0; q < QMAX; ++q) {
        key[q] = INT_MAX; slot[q] = 0;
        if (q < per) {
            if (!isnan(bdx[q])) {
                const double dx = bdx[q], dy = bdy[q];
                const double qx = ex + c * dx - s * dy;                             // :169
                const double qy = ey + s * dx + c * dy;                             // :170
                // (a reciprocal multiply with an exact-division guard, as window_map_index's, measured no faster: 173.9 vs 166.9 us
                // at 1081 beams -- the kernel is a chain of barriers and LDS round trips, not instruction issue)
                const int cx = (int)((qx - fr.xlo) / lv.step);                      // :174
                const int cy = (int)((qy - fr.ylo) / lv.step);                      // :175
                const int x0 = cx - nc, y0 = cy - nc;
                if (x0 < 0 || y0 < 0 || cx + nc >= fr.fw || cy + nc >= fr.fh) bad = true;
                else key[q] = (y0 << 16) | x0;              // (fmax < 2^15 since fmax * fpitch < 2^29; no integer division to get them back)
            }
        }
    }
    __syncthreads();
    DBG_CLOCK(41, it == 0 && p == 0);
#pragma unroll
    for (int q = 0; q < QMAX; ++q) {
        if (key[q] == INT_MAX) continue;
        cell_set_insert(hkey, hmask, key[q], slot[q]);
        atomicMin(&hown[slot[q]], q * NT + tid);
        if (mark) {                                        // tiles of the (2 nc + 1)^2 patch at (x0, y0)
            const int y0 = key[q] >> 16, x0 = key[q] & 0xFFFF;
            const int tx0 = x0 >> BLUR_SHIFT, ty0 = y0 >> BLUR_SHIFT;
            const int cx = (((x0 & (BLUR_TILE - 1)) + span) >> BLUR_SHIFT) - ntl;
            const int cy = (((y0 & (BLUR_TILE - 1)) + span) >> BLUR_SHIFT) - ntl;
            uint32_t* w = corner_s + ((cy * 2 + cx) * lv.tmax + ty0) * wp + (tx0 >> 5);
            const uint32_t m = 1u << (tx0 & 31);
            // neighbouring beams share the corner tile: a plain read first, the atomic only for a new bit
            if (!(*w & m)) atomicOr(w, m);
        }
    }
    __syncthreads();
    DBG_CLOCK(42, it == 0 && p == 0);
    // ordered compaction, beam order = (q, wave, lane): per (q, wave) survivor counts through ballots, one barrier, then
    // every survivor's position = survivors of the steps / waves before + survivors of lower lanes of its own ballot
    const int wv = tid >> 6, lane = tid & 63;
    const unsigned long long below = lane ? (~0ull >> (64 - lane)) : 0ull;
    int* qcnt = cnt_s;                                      // [per][4] counts (per <= 8: 32 ints)
    unsigned owner = 0u;                                    // bit q: this thread's beam of step q owns its cell
#pragma unroll
    for (int q = 0; q < QMAX; ++q) {
        if (q < per) {
            const bool k = key[q] != INT_MAX && hown[slot[q]] == q * NT + tid;
            owner |= (k ? 1u : 0u) << q;
            const unsigned long long km = __ballot(k);
            if (lane == 0) qcnt[q * NW + wv] = __popcll(km);
        }
    }
    __syncthreads();
    int* out = lv.cells + ((size_t)p * lv.ntheta + it) * lv.kmax;
    int* pout = lv.bnb ? lv.pcells + ((size_t)p * lv.ntheta + it) * lv.kmax : nullptr;
    const int gp = lv.tmax << 2;
    int run = 0, pos_end = 0;
#pragma unroll
    for (int q = 0; q < QMAX; ++q) {
        if (q < per) {
            int before = run;
            for (int w2 = 0; w2 < NW; ++w2) { const int c2 = qcnt[q * NW + w2]; if (w2 < wv) before += c2; run += c2; }
            const unsigned long long km = __ballot((owner >> q) & 1u);
            if ((owner >> q) & 1u) {
                const int pos = before + __popcll(km & below);
                if (pos < lv.kmax) {
                    const int y0 = key[q] >> 16, x0 = key[q] & 0xFFFF;
                    out[pos] = y0 * lv.fpitch + x0;
                    if (pout) {                                // the block of the patch corner, as a byte offset into gmin2
                        const int Y0 = y0 >> 2, X0 = x0 >> 2;
                        pout[pos] = (Y0 * gp + X0) * 4;
                        if (lv.bnb == 2) {                     // ... and into the phase planes of gmin3d
                            const int hp = gp >> 1;
                            lv.p3cells[((size_t)p * lv.ntheta + it) * lv.kmax + pos] = ((((Y0 & 1) << 1 | (X0 & 1)) * hp + (Y0 >> 1)) * hp + (X0 >> 1)) * 4;
                        }
                    }
                }
            }
        }
    }
    pos_end = run;
    const int pos = pos_end;
    DBG_CLOCK(43, it == 0 && p == 0);
    if (tid == NT - 1) {
        int K = pos;                                       // the last thread ends at the total
        if (K > lv.kmax) { K = lv.kmax; bad = true; }
        lv.kcount[p * lv.ntheta + it] = K;
    }
  }
    if (bad) atomicOr(&flags[p], SLAM2D_F_ENDPOINT_OUTSIDE);
    if (!mark) return;                                     // (block-uniform)
    __syncthreads();                                       // the corner bits of the block's angles are all set
    {
        const int nitem = lv.tmax * wp;
        for (int i = tid; i < 2 * nitem; i += NT) {      // horizontal: class cx covers tx0 .. tx0 + ntl + cx
            const int cy = i / nitem, rj = i - cy * nitem, j = rj % wp;
            unsigned long long d = 0ull;
#pragma unroll
            for (int cx = 0; cx < 2; ++cx) {
                const uint32_t* c = corner_s + (cy * 2 + cx) * nitem + rj;
                unsigned long long v = ((unsigned long long)c[0] << 32) | (j ? c[-1] : 0u);
                for (int k = 0; k < ntl + cx; ++k) v |= v << 1;
                d |= v;
            }
            hd_s[i] = (uint32_t)(d >> 32);
        }
        __syncthreads();
        for (int i = tid; i < nitem; i += NT) {          // vertical: class cy covers ty0 .. ty0 + ntl + cy; then to the particle's bitmap
            const int row = i / wp, j = i - row * wp;
            uint32_t v = 0u;
            for (int dy = 0; dy <= ntl + 1 && dy <= row; ++dy) {
                if (dy <= ntl) v |= hd_s[i - dy * wp];
                v |= hd_s[nitem + i - dy * wp];
            }
            const int left = lv.tmax - 32 * j;             // tiles of this word inside the row
            if (left < 32) v &= (1u << left) - 1u;
            if (v) {
                const int start = row * lv.tmax + 32 * j, sh = start & 31;
                const uint32_t lo = v << sh, hi = sh ? v >> (32 - sh) : 0u;
                if (lo) atomicOr(&lin_s[start >> 5], lo);
                if (hi) atomicOr(&lin_s[(start >> 5) + 1], hi);
            }
        }
        __syncthreads();
        for (int i = tid; i < nneed; i += NT) need_g[i] = lin_s[i];
    }
}

// ------------------------------------------------------------------------------------
// K1c  pose-cube sweep                              (Utils/ScanMatcher_OGBased.py:116-132)
//      score[theta][dy][dx] = sum_k field[cy_k + dy][cx_k + dx] + rv + thetaWeight
//
//      One BLOCK scores 64 slots of 4 consecutive dx of one (particle, theta), one slot per lane (two to four
//      slots per lane measured slower in round 1, config 2: 132-134 us against 124 us): lanes run along the
//      flattened (dy, dx/4) plane, so every gather of a wave is a few contiguous row segments of the
//      fixed-point uint32 field; its 4 waves split the unique-cell list.  The list is wave-uniform: it is
//      read with scalar loads and the field through a buffer resource as (per-lane constant VGPR offset) +
//      (scalar cell offset), 16 bytes per lane.  The cube's shape and slots, the exact sums (Acc4), the score
//      expression, the plane's partial, the XCD pinning and the match record come from the exact-score core above
//      (cube_of .. store_match), which K1d, K1e and k_moments read as well.
// ------------------------------------------------------------------------------------
// A "slot" is 4 consecutive dx of one dy row (the last slot of a row is partly padding); one lane
// scores one slot, i.e. each gather is one 16-byte buffer load -- a quarter of the vector-memory
// instructions of a dword-per-lane sweep for the same bytes.
// One BLOCK = 64 slots of one (particle, theta); its 4 waves score the SAME slots against
// interleaved quarters of the cell list (wave s takes cells s, s+4, ...), so four waves stream through
// the same field rows at the same time -- one L1 working set per block (measured 124 -> 117 us; the
// gathers run at L1 delivery rate, bypassing L1 costs 1.6x) -- and their exact integer partial sums
// meet in LDS.
#define SWEEP_REST_CHUNKS 4
#ifndef SWEEP_MAIN_CHUNKS
#define SWEEP_MAIN_CHUNKS 1
#endif
#ifndef SWEEP_DEPTH
#define SWEEP_DEPTH 8
#endif
#define SWEEP_DEEP_MAX_BLOCKS 64     // blocks per particle up to which the launch is about one round of blocks (latency-bound): the deep loop
// arg-max, confidence and matched pose of particle p from the sweep's partials (k_select<0> without the soft-max draw), by ONE
// wave -- the sweep's last-arriving block of the particle (k_sweep, sel_out).  The partials were published with write-through
// stores by other blocks: they are read past this CU's L1.
__device__ __forceinline__ Slam2dPartial load_partial_through(const Slam2dPartial* src) {
    const unsigned long long* u = reinterpret_cast<const unsigned long long*>(src);
    const unsigned long long a = __hip_atomic_load(u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const unsigned long long b = __hip_atomic_load(u + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const unsigned long long c = __hip_atomic_load(u + 2, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    Slam2dPartial pt;
    pt.max = __longlong_as_double((long long)a); pt.sumexp = __longlong_as_double((long long)b);
    pt.argmax = (int)(unsigned)c; pt.has_nan = (int)(c >> 32);
    return pt;
}
__device__ __forceinline__ void select_argmax_from_partials(const Slam2dLevel& lv, const int p, const int nW, const double* __restrict__ est,
                                                            const int estride, Slam2dMatch* out) {
    const Slam2dPartial* pt0 = lv.partials + (size_t)p * lv.npartial;
    const PartialsTotal t = partials_total(nW, [&](const int w) { return load_partial_through(pt0 + w); });
    if ((threadIdx.x & 63) == 0) {
        const double* e = est + (size_t)p * estride;
        store_match(lv, p, e[0], e[1], e[2], lv.thetas[t.best.i / cube_of(lv).npose], t.best.i, t.best.i, t.best.v, t.total, out);
    }
}

template <int mode, bool SKIP>
// (whole cube, no skip test: 8 waves per SIMD -- 64 VGPRs instead of 66 -- hold the reference's fine level, 30 blocks per
// particle x 64 particles = 1 920 blocks of 4 waves, in ONE round of blocks instead of a full one and a sliver)
__global__ __launch_bounds__(256, (mode == 0 && !SKIP) ? 8 : 1) void k_sweep(Slam2dLevel lv, int P, int chunks, int bpp, const double* __restrict__ sel_est = nullptr,
                                               int sel_estride = 0, Slam2dMatch* sel_out = nullptr, int deep = 0) {
    // mode 0: the whole cube.  mode 1: only the slots of the prior's ring (lv.ring).  mode 2: the
    // whole cube, for the particles the ring pass could not settle (lv.prune_state[p] != 0) -- see write_priors.
    // SKIP: a wave-load whose whole patch (its 6-7 pose rows x all dx, at the cell) lies in tiles that
    // hold the free-space constant is not issued; the constant is added once per skipped cell at the end
    // (integer sums: exact).  ~29 % of the loads at config 2.
    __shared__ unsigned long long part_s[3][WAVE * 4];
    __shared__ unsigned long long free_s[64];
    int p, w;
    xcd_particle(blockIdx.x, bpp, &p, &w);
    if (p >= P) return;
    if (mode == 2 && lv.prune_state[p] == 0) return;
    if (mode == 1 && lv.prune_state[p] != 0) return;
    if constexpr (SKIP) {
        if (threadIdx.x < 64) free_s[threadIdx.x] = lv.freerow[(size_t)p * 64 + threadIdx.x];
        __syncthreads();
    }
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    // modes 0 / 1: one block per (theta, chunk).  mode 2: one block per (theta, SWEEP_REST_CHUNKS chunks), so that
    // the launch -- empty for every settled particle -- is a quarter of the blocks
    constexpr int CPB = mode == 2 ? SWEEP_REST_CHUNKS : (mode == 0 ? SWEEP_MAIN_CHUNKS : 1);      // chunks per block
    const int groups = (chunks + CPB - 1) / CPB;
    const int it = w / groups;
    const Cube cube = cube_of(lv);
    const int nx = cube.nx, npose = cube.npose, nq = cube.nq, nslot = cube.nslot;
    const int* __restrict__ cl = lv.cells + ((size_t)p * lv.ntheta + it) * lv.kmax;
    const int K = lv.kcount[p * lv.ntheta + it];
    const int nring = mode == 1 ? lv.ring[0] : 0;
    if (mode == 1 && (w - it * groups) * WAVE >= nring) return;     // also nring = -1: the ring did not fit
    // address = field base + per-lane byte offset (constant over k) + wave-uniform byte offset (the cell)
    const __amdgpu_buffer_rsrc_t rsrc = field_rsrc(lv, p);
    const int dbg0 = lv.fine ? 44 : 32;
    auto sweep_chunk = [&](const int ch) {
    DBG_CLOCK(dbg0, p == 0 && it == 0 && ch == 0);
    int u = ch * WAVE + lane;             // the lane's slot
    if (mode == 1) u = u < nring ? lv.ring[1 + u] : nslot;
    const Slot sl = slot_of(cube, lv.fpitch, u);
    const int off = sl.off, q0 = sl.q0, nv = sl.nv;
    Acc4 acc;
    unsigned nfree = 0u;
    if constexpr (SKIP) {
        // This wave's cells (k = wave, wave + 4, ...) 64 at a time, one per lane; the loop then pops cells off a
        // ballot mask and fetches their offsets with v_readlane, SWEEP_DEPTH loads in flight per wave -- no
        // memory access and no divergent branch in the dependency chain.  The patch test (vector code, outside
        // the load loop) removes the cells whose patch holds only the free-space constant.
        const int r_lo = (ch * WAVE) / nq, r_hi = min(nx - 1, (ch * WAVE + WAVE - 1) / nq), ncols = 4 * nq;
        const double inv_pitch = 1.0 / (double)lv.fpitch;
        for (int base = wave; base < K; base += 4 * WAVE) {
            const int kk = base + 4 * lane;
            const bool valid = kk < K;
            const int cof = valid ? cl[kk] : 0;
            int y0 = (int)((double)cof * inv_pitch);                // cof / fpitch without the integer division
            if (y0 * lv.fpitch > cof) --y0;
            if ((y0 + 1) * lv.fpitch <= cof) ++y0;
            const int x0 = cof - y0 * lv.fpitch;
            bool load = valid;
            {
                const int tx0 = x0 >> BLUR_SHIFT, tx1 = (x0 + ncols - 1) >> BLUR_SHIFT;
                const unsigned long long need = ((2ull << (tx1 - tx0)) - 1ull) << tx0;
                const unsigned long long f = free_s[(y0 + r_lo) >> BLUR_SHIFT] & free_s[(y0 + r_hi) >> BLUR_SHIFT];
                load = valid && (~f & need) != 0ull;
                nfree += (unsigned)__popcll(__ballot(valid && !load));
            }
            unsigned long long todo = __ballot(load);
            const int boff = cof * 4;
            while (todo) {
                int c[SWEEP_DEPTH];
#pragma unroll
                for (int i = 0; i < SWEEP_DEPTH; ++i) {
                    c[i] = 0x7ffffff0;                             // beyond the buffer: reads zeros
                    if (todo) {
                        const int j = __ffsll((long long)todo) - 1;
                        todo &= todo - 1;
                        c[i] = __builtin_amdgcn_readlane(boff, j);
                    }
                }
                u32x4 v[SWEEP_DEPTH];
#pragma unroll
                for (int i = 0; i < SWEEP_DEPTH; ++i) v[i] = __builtin_amdgcn_raw_buffer_load_b128(rsrc, off, c[i], 0);
#pragma unroll
                for (int i = 0; i < SWEEP_DEPTH; ++i) acc.add(v[i]);
            }
        }
    } else if (deep) {
        // Round 4: a level whose launch is ONE round of blocks (the reference's 11 x 11 fine cube: 30 blocks per particle) is
        // bound by the latency of this loop, not by the gathers' throughput -- with two loads in flight a wave's ~40 cells were
        // ~20 round trips.  The wave's cells come in one vector load (a lane each), v_readlane hands them to the loop as scalar
        // offsets, SWEEP_DEPTH loads are in flight (the skip loop's structure without its patch test).
        for (int base = wave; base < K; base += 4 * WAVE) {
            const int kk = base + 4 * lane;
            const int boff = kk < K ? cl[kk] * 4 : 0x7ffffff0;                     // beyond the buffer: reads zeros
            const int n = min(WAVE, (K - base + 3) >> 2);                           // this wave's cells in this batch (wave-uniform)
            for (int j0 = 0; j0 < n; j0 += SWEEP_DEPTH) {
                int c[SWEEP_DEPTH];
#pragma unroll
                for (int i = 0; i < SWEEP_DEPTH; ++i) c[i] = __builtin_amdgcn_readlane(boff, min(j0 + i, WAVE - 1));
                u32x4 v[SWEEP_DEPTH];
#pragma unroll
                for (int i = 0; i < SWEEP_DEPTH; ++i) v[i] = __builtin_amdgcn_raw_buffer_load_b128(rsrc, off, j0 + i < n ? c[i] : 0x7ffffff0, 0);
#pragma unroll
                for (int i = 0; i < SWEEP_DEPTH; ++i) acc.add(v[i]);
            }
        }
    } else {
#pragma unroll 2
    for (int k = wave; k < K; k += 4) {
        const int cell = cl[k] * 4;
        acc.add(__builtin_amdgcn_raw_buffer_load_b128(rsrc, off, cell, 0));
    }
    }
    if constexpr (SKIP) {                                  // the skipped cells: each adds the free-space cost
        const double fv = lv.floor_value;
        const unsigned long long add = (unsigned long long)nfree * (fv > 0.5 * fv ? 0u : (uint32_t)rint(-fv * lv.cost_scale));
#pragma unroll
        for (int e = 0; e < 4; ++e) acc.add_u64(e, add);
    }
    DBG_CLOCK(dbg0 + 1, p == 0 && it == 0 && ch == 0);
    if (wave > 0) {
#pragma unroll
        for (int e = 0; e < 4; ++e) part_s[wave - 1][e * WAVE + lane] = acc.get(e);
    }
    __syncthreads();
    DBG_CLOCK(dbg0 + 2, p == 0 && it == 0 && ch == 0);
    if (wave > 0) return;
    {
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const int ix = e * WAVE + lane;
        acc.add_u64(e, part_s[0][ix] + part_s[1][ix] + part_s[2][ix]);
    }
    double* __restrict__ out = lv.cube + ((size_t)p * lv.ntheta + it) * npose;
    const double inv = 1.0 / lv.cost_scale;
    double sc[4], prv[4], ptw[4];
    Best me{-INFINITY, INT_MAX, 0};
    slot_priors(lv.prior + (size_t)p * 2 * npose, cube, q0, prv, ptw);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        sc[e] = -INFINITY;
        if (e < nv) {
            const int q = q0 + e;
            sc[e] = pose_score(acc.get(e), inv, prv[e], ptw[e]);
            out[q] = sc[e];
            Best cand{sc[e], it * npose + q, isnan(sc[e]) ? 1 : 0};
            if (better(cand, me)) me = cand;
        }
    }
    // the chunk's partial for k_select (lane = one slot: indices ascend with the lane)
    const Slam2dPartial pt = plane_partial(me, sc, nv);
    if (lane == 0) {
        Slam2dPartial* dst = lv.partials + (size_t)p * lv.npartial + it * chunks + ch;
        if (mode == 0 && sel_out != nullptr) {             // (the particle's last block reads it in this launch: write-through)
            unsigned long long* u = reinterpret_cast<unsigned long long*>(dst);
            __hip_atomic_store(u, (unsigned long long)__double_as_longlong(pt.max), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __hip_atomic_store(u + 1, (unsigned long long)__double_as_longlong(pt.sumexp), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __hip_atomic_store(u + 2, ((unsigned long long)(unsigned)pt.has_nan << 32) | (unsigned)pt.argmax, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        } else {
            *dst = pt;
        }
    }
    DBG_CLOCK(dbg0 + 3, p == 0 && it == 0 && ch == 0);
    }
    };
    if constexpr (CPB > 1) {
        const int c0 = (w - it * groups) * CPB;
        for (int ch = c0; ch < min(chunks, c0 + CPB); ++ch) {
            sweep_chunk(ch);
            __syncthreads();                               // part_s is reused by the next chunk
        }
    } else {
        sweep_chunk(w - it * groups);
    }
    if constexpr (mode == 0) {
        // Round 4 (sel_out != NULL: a level matched by arg-max, i.e. no soft-max draw, which would need the cube): the block takes a
        // ticket from the particle's third arrival counter once its partials are out, and the particle's LAST block selects --
        // k_select's work without its launch.
        if (sel_out != nullptr && wave == 0) {
            // (publish / consume as in k_exact_select: the partials left as relaxed agent-scope 8-byte atomic stores, are drained here
            // and read back by the last block with load_partial_through's agent-scope atomic loads -- MI355X_MICROARCH.md's "8-B agent
            // atomics both sides"; no cache to write back or invalidate on either side)
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            __atomic_signal_fence(__ATOMIC_SEQ_CST);
            unsigned ticket = 0u;
            if (lane == 0) ticket = __hip_atomic_fetch_add(&lv.sync[p * SLAM2D_SYNC_WORDS + 2], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            ticket = (unsigned)__builtin_amdgcn_readfirstlane((int)ticket);
            if (ticket == (unsigned)(bpp - 1)) {
                if (lane == 0) __hip_atomic_store(&lv.sync[p * SLAM2D_SYNC_WORDS + 2], 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                __atomic_signal_fence(__ATOMIC_SEQ_CST);
                select_argmax_from_partials(lv, p, lv.ntheta * chunks, sel_est, sel_estride, sel_out);
            }
        }
    }
}

// Small cubes (a plane of <= 32 slots of 4 dx: 2*ncell+1 <= 7, e.g. the 5 x 5 fine level behind a coarse factor of 2):
// k_sweep would leave most lanes of its waves without a slot.  Here ONE wave scores a whole (particle, theta) plane:
// lane = (slot, cell slice) -- floor(64 / slots) slices share the cell list, which is staged in LDS once (no
// vector-memory instruction per cell for the list), so a plane costs ~K / slices 16-byte gathers instead of K.
// Same exact integer sums, same cube / partial layout as k_sweep with one chunk per theta.
// One (particle, theta) plane of a small cube by one wave; returns the plane's reduction (to every lane) and stores the scores
// and, with `write`, the plane's Slam2dPartial.  small_lds: [64 * 4] partial sums, then [kmax] cells.
// NWAVES waves (one block) split the cell list; the scores, the reduction and the return value are wave 0's.
// small_lds: [NWAVES * 4 * 64] partial sums, then [kmax] cells.
template <int NWAVES>
__device__ __forceinline__ Best sweep_small_plane(const Slam2dLevel& lv, const int p, const int it, unsigned long long* small_lds,
                                                  const bool write) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const Cube cube = cube_of(lv);
    const int npose = cube.npose, nslot = cube.nslot;           // nslot <= 32 (checked by the host)
    const int S = WAVE / nslot;                                 // cell slices per wave
    const int K = lv.kcount[p * lv.ntheta + it];
    const int* __restrict__ cl = lv.cells + ((size_t)p * lv.ntheta + it) * lv.kmax;
    int* cells_s = reinterpret_cast<int*>(small_lds + NWAVES * WAVE * 4);
    for (int k = threadIdx.x; k < K; k += NWAVES * WAVE) cells_s[k] = cl[k];
    const __amdgpu_buffer_rsrc_t rsrc = field_rsrc(lv, p);
    const bool active = lane < S * nslot;
    const int sl = lane / nslot;
    const Slot slot = slot_of(cube, lv.fpitch, lane % nslot);
    const int off = slot.off;
    const int ST = S * NWAVES;                                  // slices of the whole block
    Acc4 acc4;
    __syncthreads();
    for (int k = sl + S * wave; k < K; k += 8 * ST) {           // 8 gathers in flight
        int o[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) o[i] = (active && k + i * ST < K) ? off + cells_s[k + i * ST] * 4 : 0x7ffffff0;
        u32x4 v[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) v[i] = __builtin_amdgcn_raw_buffer_load_b128(rsrc, o[i], 0, 0);
#pragma unroll
        for (int i = 0; i < 8; ++i) acc4.add(v[i]);
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) small_lds[(wave * 4 + e) * WAVE + lane] = acc4.get(e);
    __syncthreads();
    Best me{-INFINITY, INT_MAX, 0};
    if (NWAVES > 1 && wave != 0) return me;
    double* __restrict__ out = lv.cube + ((size_t)p * lv.ntheta + it) * npose;
    const double inv = 1.0 / lv.cost_scale;
    const int nv = lane < nslot ? slot.nv : 0, q0 = slot.q0;
    double sc[4], prv[4], ptw[4];
    slot_priors(lv.prior + (size_t)p * 2 * npose, cube, q0, prv, ptw);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        sc[e] = -INFINITY;
        if (e < nv) {
            unsigned long long acc = 0ull;
            for (int w2 = 0; w2 < NWAVES; ++w2)
                for (int s2 = 0; s2 < S; ++s2) acc += small_lds[(w2 * 4 + e) * WAVE + lane + s2 * nslot];
            const int q = q0 + e;
            sc[e] = pose_score(acc, inv, prv[e], ptw[e]);
            if (write) out[q] = sc[e];
            Best cand{sc[e], it * npose + q, isnan(sc[e]) ? 1 : 0};
            if (better(cand, me)) me = cand;
        }
    }
    if (!write) return wave_best_ordered(me);
    const Slam2dPartial pt = plane_partial(me, sc, nv);
    if (lane == 0) lv.partials[(size_t)p * lv.npartial + it] = pt;
    return Best{pt.max, pt.argmax, pt.has_nan};
}
// pruned != 0 (Slam2dLevel.bnb == 3, "angle bounds"): a plane whose upper bound (k_abound) lies more than SLAM2D_BNB_MARGIN
// below the particle's seed score (k_aseed) is not scored -- it cannot hold the arg-max and all such planes together change
// the confidence by < ntheta * 25 * exp(-30) relative; its partial says "nothing here".
__global__ __launch_bounds__(64) void k_sweep_small(Slam2dLevel lv, int P, int pruned) {
    extern __shared__ __attribute__((aligned(16))) unsigned long long small_lds[];   // [64 * 4] partial sums, then [kmax] cells
    int p, it;
    xcd_particle(blockIdx.x, lv.ntheta, &p, &it);
    if (p >= P) return;
    if (pruned && !(lv.bounds[(size_t)p * lv.ntheta + it] >= unorder_bits(lv.bnb_best[p]) - SLAM2D_BNB_MARGIN)) {
        if (threadIdx.x == 0) {
            Slam2dPartial pt;
            pt.max = -INFINITY; pt.sumexp = 0.0; pt.argmax = INT_MAX; pt.has_nan = 0;
            lv.partials[(size_t)p * lv.npartial + it] = pt;
        }
        return;
    }
    sweep_small_plane<1>(lv, p, it, small_lds, true);
}

// Angle bounds (Slam2dLevel.bnb == 3; cubes of <= 7 x 7 poses per angle behind long cell lists, e.g. the 5 x 5 fine level of a
// 1081-beam scan).  All poses of one angle read, at endpoint cell k, a window of <= 7 x 7 field cells that starts at the patch
// corner; for windows of <= 5 x 5 cells it lies inside the aligned 8 x 8 block gmin2 summarises at (corner >> 2), so
//     U(theta) = -(sum_k gmin2[cell k] << 12) / cost_scale + max(rv + thetaWeight)
// bounds every pose of the plane: ONE 4-byte load per cell and angle, 64 cells per load instruction -- against one 16-byte
// gather per cell and 6 poses in the exact sweep, whose time is L1 tag lookups (30 sectors per load).  One wave per
// (particle, theta); the particle's best bound (packed with its theta) goes to seed_key for k_aseed.
#ifndef ABOUND_STRIDE
#define ABOUND_STRIDE 1
#endif
// (ABOUND_WAVES angles per block: a launch of one-wave blocks pays ~4.5 ns of dispatch per block whatever they do -- 8 896 blocks at
// config 5, 40-50 us for ten gathers per wave; round 6)
#ifndef ABOUND_WAVES
#define ABOUND_WAVES 16
#endif
__global__ __launch_bounds__(64 * ABOUND_WAVES) void k_abound(Slam2dLevel lv, int P) {
    const int ngrp = (lv.ntheta + ABOUND_WAVES - 1) / ABOUND_WAVES;
    int p, grp;
    xcd_particle(blockIdx.x, ngrp, &p, &grp);
    const int it = grp * ABOUND_WAVES + (threadIdx.x >> 6);
    if (p >= P || it >= lv.ntheta) return;
    const int lane = threadIdx.x & 63;
    const int npose = cube_of(lv).npose;
    const int gp = lv.tmax << 2;
    const int K = lv.kcount[p * lv.ntheta + it];
    const int* __restrict__ pcl = lv.pcells + ((size_t)p * lv.ntheta + it) * lv.kmax;
    const __amdgpu_buffer_rsrc_t rg2 = image_rsrc(lv.gmin2 + (size_t)p * gp * gp, (size_t)gp * gp * sizeof(uint32_t));
    // (Every term of the bound is <= 0, so leaving cells out keeps it an upper bound -- but using every 4th cell of the list
    // already made it too loose to prune anything at config 5: the exact sweep went from 32 back to 156 us.  Stride 1.)
    unsigned sum = 0u;                                     // 20-bit values, <= 2048 cells: no carry
    const int Ks = (K + ABOUND_STRIDE - 1) / ABOUND_STRIDE;
    for (int k0 = 0; k0 < Ks; k0 += WAVE * 8) {
        int off[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) { const int k = k0 + i * WAVE + lane; off[i] = k < Ks ? pcl[k * ABOUND_STRIDE] : 0x7ffffff0; }
        unsigned v[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) v[i] = __builtin_amdgcn_raw_buffer_load_b32(rg2, off[i], 0, 0);
#pragma unroll
        for (int i = 0; i < 8; ++i) sum += v[i];
    }
    sum = row16_sum_u32(sum);
    const unsigned tot = (unsigned)__builtin_amdgcn_readlane((int)sum, 0) + (unsigned)__builtin_amdgcn_readlane((int)sum, 16) +
                         (unsigned)__builtin_amdgcn_readlane((int)sum, 32) + (unsigned)__builtin_amdgcn_readlane((int)sum, 48);
    // largest prior of the plane (+inf when one is NaN: np.argmax returns the first NaN, such a plane is always scored)
    double pmx = 0.0;
    if (!lv.fine) {
        const double* __restrict__ pr = lv.prior + (size_t)p * 2 * npose;
        pmx = -INFINITY;
        for (int q = lane; q < npose; q += WAVE) { const double v = pr[q] + pr[npose + q]; pmx = isnan(v) ? INFINITY : fmax(pmx, v); }
        pmx = wave64_max(pmx);
    }
    const double U = (-(((double)tot * 4096.0) / lv.cost_scale) + pmx) + 1e-9;
    if (lane == 0) {
        lv.bounds[(size_t)p * lv.ntheta + it] = U;
        if (U > -INFINITY && U < INFINITY) atomicMax(&lv.seed_key[p], (order_bits(U) & ~0x3FFFull) | (unsigned long long)it);
        else if (U == INFINITY) atomicMax(&lv.seed_key[p], (order_bits(1e300) & ~0x3FFFull) | (unsigned long long)it);
    }
}
// The seed: the plane of the particle's best-bound angle, exactly; its best score is a lower bound of the cube's maximum.  One
// 1024-thread block per particle (16 waves share the cell list: a lone wave took ~30 us for 900 cells).
#define ASEED_WAVES 16
__global__ __launch_bounds__(64 * ASEED_WAVES) void k_aseed(Slam2dLevel lv, int P) {
    extern __shared__ __attribute__((aligned(16))) unsigned long long small_lds[];
    const int p = blockIdx.x;
    const unsigned long long key = lv.seed_key[p];
    double best = -INFINITY;                               // no finite bound anywhere: no threshold, every plane is scored
    if (key) {                                             // (block-uniform)
        const Best me = sweep_small_plane<ASEED_WAVES>(lv, p, (int)(key & 0x3FFF), small_lds, false);
        if (!me.nan && me.i != INT_MAX) best = me.v;
    }
    if (threadIdx.x == 0) lv.bnb_best[p] = order_bits(best);
}

// ------------------------------------------------------------------------------------
// K1d  arg-max / soft-max draw / confidence / matched pose   (Utils/ScanMatcher_OGBased.py:133-143)
//      one wave per particle, working on the per-wave partials of the sweep
// ------------------------------------------------------------------------------------
template <int mode>
__global__ __launch_bounds__(64) void k_select(Slam2dLevel lv, int chunks, const double* __restrict__ est,
                                               int estride, const double* __restrict__ uniform, Slam2dMatch* out) {
    // mode as in k_sweep.  In mode 1 only the first ceil(ring length / 64) chunks of every theta hold
    // partials; the partial of (theta it, chunk ch) sits at it * chunks + ch in every mode.
    const int p = blockIdx.x, lane = threadIdx.x;
    const Cube cube = cube_of(lv);
    const int nx = cube.nx, npose = cube.npose;
    if (mode == 2 && lv.prune_state[p] == 0) return;
    if (mode == 1 && lv.prune_state[p] != 0) return;
    const int nring = mode == 1 ? lv.ring[0] : 0;
    if (mode == 1 && nring < 0) { if (lane == 0) lv.prune_state[p] = 1; return; }
    const int vch = mode == 1 ? (nring + WAVE - 1) / WAVE : chunks;          // chunks that hold partials
    const int nW = lv.ntheta * vch;
    const Slam2dPartial* __restrict__ pt0 = lv.partials + (size_t)p * lv.npartial;
    auto part = [&](const int v) -> const Slam2dPartial& { return pt0[(v / vch) * chunks + (v % vch)]; };
    const double* __restrict__ c = lv.cube + (size_t)p * lv.ntheta * npose;
    // global max / argmax; total = sum_w sumexp_w * exp(max_w - M)
    const PartialsTotal pt = partials_total(nW, part);
    const Best me = pt.best;
    const double M = me.v, mine = pt.mine, incl = pt.incl, total = pt.total;
    if (mode == 1) {
        // a pose outside the ring scores rv + (field sum) + thetaWeight <= -100 + K * (largest field value);
        // K = cells of its theta, so the fewest cells of any theta give the bound for all of them
        int kmin = INT_MAX;
        for (int it = lane; it < lv.ntheta; it += WAVE) kmin = min(kmin, lv.kcount[p * lv.ntheta + it]);
        for (int o = 1; o < WAVE; o <<= 1) kmin = min(kmin, __shfl_xor(kmin, o));
        const double outside = -100.0 + (double)kmin * lv.frames[p].field_max;
        if (!(M >= outside + SLAM2D_PRUNE_MARGIN)) {     // also NaN: the ring alone does not settle this particle
            if (lane == 0) lv.prune_state[p] = 1;
            return;
        }
    }
    const int per = (nW + WAVE - 1) / WAVE;           // partials per lane
    int pick = me.i;
    if (uniform != nullptr && !isnan(total)) {
        // np.random.choice(n, 1, p): first index whose normalised cdf exceeds u (:137-138)
        const double target = uniform[p] * total;
        const unsigned long long ahead = __ballot(incl > target);
        const int lsel = ahead ? __ffsll((long long)ahead) - 1 : WAVE - 1;
        double run = readlane_f64(incl - mine, lsel);             // cdf before lane lsel's partials
        const int s0 = min(lsel * per, nW - 1), s1 = max(s0 + 1, min(nW, lsel * per + per));
        int wsel = s1 - 1;
        for (int w = s0; w < s1; ++w) {                           // wave-uniform loop
            const double t = part(w).sumexp * exp(part(w).max - M);
            if (run + t > target || w == s1 - 1) { wsel = w; break; }
            run += t;
        }
        const int it = wsel / vch, ch = wsel - it * vch;
        const int nslot = cube.nslot;
        if (mode == 1) {
            // ring chunk: lane l owns slot ring[ch*64 + l] = up to 4 consecutive poses; slots ascend with l,
            // so the lanes walk the chunk's poses in cube order
            const int idx = ch * WAVE + lane;
            const Slot sl = slot_of(cube, lv.fpitch, idx < nring ? lv.ring[1 + idx] : nslot);
            const int q0 = sl.q0, nvl = sl.nv;
            double lsum = 0.0;
            for (int e = 0; e < nvl; ++e) lsum += exp(c[(size_t)it * npose + q0 + e] - M);
            const double linc = wave_scan_incl_f64(lsum);
            const unsigned long long hit = __ballot(nvl > 0 && run + linc > target);
            const unsigned long long have = __ballot(nvl > 0);
            const int llast = 63 - __clzll((long long)have);                      // chunk's last slot (have != 0)
            const int l2 = hit ? __ffsll((long long)hit) - 1 : llast;
            double r2 = run + readlane_f64(linc - lsum, l2);
            int found = -1;
            if (lane == l2) {
                for (int e = 0; e < nvl; ++e) {
                    r2 += exp(c[(size_t)it * npose + q0 + e] - M);
                    if (r2 > target) { found = it * npose + q0 + e; break; }
                }
                if (found < 0) found = it * npose + q0 + max(0, nvl - 1);         // rounding fallback: last pose
            }
            pick = __builtin_amdgcn_readlane(found, l2);
        } else {
        // inside chunk wsel: it covers slots [ch*64, ...) = a contiguous pose range [qlo, qhi);
        // lane l owns a contiguous run of `per2` poses of it
        auto first_pose = [&](const int s) { return s < nslot ? slot_of(cube, lv.fpitch, s).q0 : npose; };
        const int qlo = first_pose(ch * WAVE), qhi = first_pose((ch + 1) * WAVE);
        const int per2 = (qhi - qlo + WAVE - 1) / WAVE;
        const int a0 = qlo + lane * per2, a1 = min(qhi, a0 + per2);
        double lsum = 0.0;
        for (int q = a0; q < a1; ++q) lsum += exp(c[(size_t)it * npose + q] - M);
        const double linc = wave_scan_incl_f64(lsum);
        const unsigned long long hit = __ballot(run + linc > target);
        pick = it * npose + max(qlo, qhi - 1);                    // rounding fallback: chunk's last pose
        if (hit) {
            const int l2 = __ffsll((long long)hit) - 1;
            double r2 = run + readlane_f64(linc - lsum, l2);
            int found = -1;
            if (lane == l2) {
                for (int q = a0; q < a1; ++q) {
                    r2 += exp(c[(size_t)it * npose + q] - M);
                    if (r2 > target) { found = it * npose + q; break; }
                }
                if (found < 0) found = it * npose + max(a0, a1 - 1);
            }
            pick = __builtin_amdgcn_readlane(found, l2);
        }
        }
    }
    if (lane == 0) {
        const double* e = est + (size_t)p * estride;
        store_match(lv, p, e[0], e[1], e[2], lv.thetas[pick / npose], pick, me.i, M, total, out);
    }
}

// ------------------------------------------------------------------------------------
// K1e  branch and bound over 4x4 pose tiles (include/slam2d.h, "Branch and bound"): the same scores as k_sweep
//      for every pose that can matter, from 1/16 of the gathers plus the exact scores of a few per cent of the tiles.
//        blur / triage  write gmin (minimum of every aligned 4x4 block of the cost image) with the field tiles;
//                  k_blur_check_redo (or k_bound_lds's prologue) derives gmin2 = min over 2x2 blocks (>> 12): a lower bound of the cost anywhere
//                  in the aligned 8x8 block that contains a pose tile's 4x4 window at a cell.
//        k_bound   one wave per (particle, theta): upper bound U of every tile (lane = one pose-tile row x 4
//                  consecutive tiles: ONE 16-byte load per cell from an image 1/16 the size of the field, 16 in
//                  flight, plain 32-bit adds); then the tile with the largest U is scored exactly and its best
//                  score raises lv.bnb_best[p] (atomic max: order-independent, deterministic).
//        k_exact   one wave per (particle, theta): every tile with U >= bnb_best - SLAM2D_PRUNE_MARGIN is scored
//                  exactly (lane = pose row x 1/16 of the cell list); ONE partial {max, argmax, sum exp} per theta.
// ------------------------------------------------------------------------------------
// exact cost sums of the 16 poses of tile (by, bx): lane = (pose row r = lane / 16, cell slice s = lane % 16) scores
// the 4 poses (4 by + r, 4 bx .. 4 bx + 3) against cells k0 + s, k0 + s + kstep, ...; on return every lane of a
// row group holds the row's 4 sums over ALL the cells this wave walked (reduced over the 16 slices).
#define EXACT_DEPTH 8
#define SLAM2D_BEAM_TABLE_MIN 512   // beams from which k_frame_axis (with its per-particle beam-endpoint table) is worth its launch
// ... and particles per launch from which it is (round 6): the merged launch makes every angle block evaluate the cos / sin of
// all beams and every scatter block the frame; when the launch fills the machine that work costs more than the two launches
// it saves (config 2: k_endpoints 57 -> 27 + 26 us at 128 particles per launch, the step 0.309 -> 0.305 ms; at 256 per launch
// 0.580 -> 0.561; at 16 per launch the two launches cost 0.113 -> 0.123)
#define SLAM2D_FRAME_KERNEL_MIN_P 128
// byte offsets of the first NPRE cells of lane slice s (cells s, s + 16, ...), beyond-the-buffer where the list ends
template <int NPRE>
__device__ __forceinline__ void tile_prefetch(const int* __restrict__ cl, const int K, int (&pre)[NPRE]) {
    const int s = threadIdx.x & 15;
#pragma unroll
    for (int i = 0; i < NPRE; ++i) pre[i] = s + 16 * i < K ? cl[s + 16 * i] * 4 : 0x7ffffff0;
}
template <int NPRE>
__device__ __forceinline__ void tile_exact(const Slam2dLevel& lv, const __amdgpu_buffer_rsrc_t rsrc, const int* __restrict__ cl,
                                           const int K, const int by, const int bx, const int (&pre)[NPRE],
                                           unsigned long long (&acc)[4]) {
    const int lane = threadIdx.x & 63, r = lane >> 4, s = lane & 15;
    const int lanepart = ((4 * by + r) * lv.fpitch + 4 * bx) * 4;
    Acc4 sum;
    {
        u32x4 v[NPRE];
#pragma unroll
        for (int i = 0; i < NPRE; ++i) v[i] = __builtin_amdgcn_raw_buffer_load_b128(rsrc, lanepart + pre[i], 0, 0);
#pragma unroll
        for (int i = 0; i < NPRE; ++i) sum.add(v[i]);
    }
    for (int k = s + 16 * NPRE; k < K; k += EXACT_DEPTH * 16) {            // longer lists
        int off[EXACT_DEPTH];
#pragma unroll
        for (int i = 0; i < EXACT_DEPTH; ++i) {
            const int kk = k + i * 16;
            off[i] = kk < K ? lanepart + cl[kk] * 4 : 0x7ffffff0;      // beyond the buffer: reads zeros
        }
        u32x4 v[EXACT_DEPTH];
#pragma unroll
        for (int i = 0; i < EXACT_DEPTH; ++i) v[i] = __builtin_amdgcn_raw_buffer_load_b128(rsrc, off[i], 0, 0);
#pragma unroll
        for (int i = 0; i < EXACT_DEPTH; ++i) sum.add(v[i]);
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) acc[e] = row16_sum_u64(sum.get(e));
}
// A seed: tile (sby, sbx) of one (particle, theta) scored exactly by one wave from the prefetched offsets `pre`; its best
// score, a lower bound of the cube's maximum, raises lv.bnb_best[p] (atomic max: order-independent, deterministic).
template <int NPRE>
__device__ __forceinline__ void tile_seed(const Slam2dLevel& lv, const int p, const int sby, const int sbx, const int* __restrict__ cl,
                                          const int K, const double inv, const int (&pre)[NPRE]) {
    const int lane = threadIdx.x & 63;
    const Cube cube = cube_of(lv);
    const int nx = cube.nx, npose = cube.npose;
    const int dy = 4 * sby + (lane >> 4);
    const bool leader = (lane & 15) == 0 && dy < nx;
    const double* __restrict__ pr = lv.prior + (size_t)p * 2 * npose;
    double prv[4], ptw[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {                           // issued ahead of the tile's field loads
        const int qq = min(dy, nx - 1) * nx + min(4 * sbx + e, nx - 1);
        prv[e] = pr[qq]; ptw[e] = pr[npose + qq];
    }
    unsigned long long acc[4];
    tile_exact<NPRE>(lv, field_rsrc(lv, p), cl, K, sby, sbx, pre, acc);
    double val = -INFINITY;
    if (leader) {
#pragma unroll
        for (int e = 0; e < 4; ++e)
            if (4 * sbx + e < nx) {
                const double sc = pose_score(acc[e], inv, prv[e], ptw[e]);
                if (!isnan(sc)) val = fmax(val, sc);
            }
    }
    val = fmax(val, __shfl_xor(val, 16));
    val = fmax(val, __shfl_xor(val, 32));
    if (lane == 0 && val > -INFINITY) atomicMax(&lv.bnb_best[p], order_bits(val));
}

// One wave per (particle, theta); blocks of a particle pinned to one XCD like the sweep's.  Lane = one pose-tile row
// x 4 consecutive tiles: ONE 16-byte load per cell.  The loop is bound by the texture path's 16 clocks per wave
// instruction (a dword-per-tile mapping needs two instructions per cell and measured 2x slower), so what counts
// is the instruction count, 1/8 of the brute-force sweep's.  The cell list is read 64 cells at a time, one per
// lane, and handed to the loads with v_readlane: no scalar-memory round trip per batch.
#define BOUND_BATCH 32
#define BOUND_GROUP 2                // waves per block = adjacent angles of one particle (measured: 1 -> 31.4 us, 2 -> 30.2, 4 -> 33.5,
//                                      8 -> 38.3 at config 2: sharing L1 lines buys little, spreading over the CUs matters)
__global__ __launch_bounds__(64 * BOUND_GROUP) void k_bound(Slam2dLevel lv, int P) {
    const int b = blockIdx.x;
    const int ngroup = (lv.ntheta + BOUND_GROUP - 1) / BOUND_GROUP;
    int p, grp;
    xcd_particle(b, ngroup, &p, &grp);
    const int it = grp * BOUND_GROUP + (threadIdx.x >> 6);
    if (p >= P || it >= lv.ntheta) return;
    const int lane = threadIdx.x & 63;
    const Cube cube = cube_of(lv);
    const int nbt = cube.nbt, nbq4 = cube.nbq4, nq = nbq4 >> 2;      // nq: lanes (of 4 tiles) per tile row
    const int gp = lv.tmax << 2;
    const int K = lv.kcount[p * lv.ntheta + it];
    const int* __restrict__ pcl = lv.pcells + ((size_t)p * lv.ntheta + it) * lv.kmax;
    const int* __restrict__ cl = lv.cells + ((size_t)p * lv.ntheta + it) * lv.kmax;
    const __amdgpu_buffer_rsrc_t rg = image_rsrc(lv.gmin2 + (size_t)p * gp * gp, (size_t)gp * gp * sizeof(uint32_t));
    DBG_CLOCK(0, b == 0);
    const bool active = lane < nbt * nq;
    const int by = lane / nq, q = lane - by * nq;
    const int voff = active ? (by * gp + 4 * q) * 4 : 0x7ffffff0;
    const double* __restrict__ pm = lv.tile_pmax + (size_t)p * nbt * nbq4;
    double pmx[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) pmx[e] = active ? pm[by * nbq4 + 4 * q + e] : -INFINITY;     // in flight during the loop
    int pre[16];
    tile_prefetch<16>(cl, K, pre);                          // for the seed tile below: likewise
    unsigned sum[4] = {0u, 0u, 0u, 0u};                    // 20-bit values, <= 2048 cells: no carry
    int cv = lane < K ? pcl[lane] : 0x7ffffff0;
    for (int base = 0; base < K; base += WAVE) {
        const int cur = cv;
        if (base + WAVE < K) cv = base + WAVE + lane < K ? pcl[base + WAVE + lane] : 0x7ffffff0;     // next 64 cells
        // (straight-line double-buffered chunks that keep 16-32 loads in flight across the whole list measured SLOWER,
        // 31.9 vs 28.4 us: the loop is bound by the L1's tag lookups -- ~19 64-byte sectors per load, 89 % hits -- not by
        // latency, and the padding loads of the last chunk are not free)
#pragma unroll
        for (int j0 = 0; j0 < WAVE; j0 += BOUND_BATCH) {
            if (base + j0 < K) {                            // (wave-uniform)
                u32x4 v[BOUND_BATCH];
#pragma unroll
                for (int i = 0; i < BOUND_BATCH; ++i)
                    v[i] = __builtin_amdgcn_raw_buffer_load_b128(rg, voff, __builtin_amdgcn_readlane(cur, j0 + i), 0);
#pragma unroll
                for (int i = 0; i < BOUND_BATCH; ++i)
#pragma unroll
                    for (int e = 0; e < 4; ++e) sum[e] += v[i][e];
            }
        }
    }
    DBG_CLOCK(1, b == 0);
    const double inv = 1.0 / lv.cost_scale;
    double* __restrict__ bnd = lv.bounds + ((size_t)p * lv.ntheta + it) * nbt * nbq4;
    Best me{-INFINITY, INT_MAX, 0};
    if (active) {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int t = by * nbq4 + 4 * q + e;
            // every pose of the tile scores (-(cost sum) / scale + rv) + thetaWeight <= -L / scale + max(rv + thetaWeight),
            // L = (sum of the block minima >> 12) << 12; 1e-9 covers the different association of the roundings;
            // padding tiles (4 q + e >= nbt) come out as -inf (their tile_pmax is)
            const double U = (-(((double)sum[e] * 4096.0) * inv) + pmx[e]) + 1e-9;
            bnd[t] = U;
            Best cand{U, t, 0};
            if (4 * q + e < nbt && better(cand, me)) me = cand;
        }
    }
    me = wave_best_ordered(me);                             // tiles ascend with the lane
    if (lv.theta_umax && lane == 0) lv.theta_umax[(size_t)p * lv.ntheta + it] = me.i != INT_MAX ? me.v : -INFINITY;
    DBG_CLOCK(2, b == 0);
    // the tile with the largest bound, exactly: its best score is a lower bound of the cube's maximum
    const int seed = me.i;
    const int sby = seed / nbq4, sbx = seed - sby * nbq4;
    tile_seed<16>(lv, p, sby, sbx, cl, K, inv, pre);
    DBG_CLOCK(3, b == 0);
    DBG_CLOCK(4, b == 0);
}

// The seed of one (particle, theta) whose cell offsets nobody has fetched yet
__device__ __forceinline__ void bound_seed_exact(const Slam2dLevel& lv, const int p, const int sby, const int sbx, const int* __restrict__ cl,
                                                 const int K, const double inv) {
    int pre[16];
    tile_prefetch<16>(cl, K, pre);
    tile_seed<16>(lv, p, sby, sbx, cl, K, inv, pre);
}

// k_bound with the particle's bound image staged in LDS (the filled-machine form: DESIGN 4).  k_bound's loop is bound by the L1's
// tag lookups -- every wave-load touches ~20 lines (11 pose-tile rows of a 2-D window), 3 160 lines per (particle, theta) -- and
// at 128-256 particles per launch it runs AT that bound (profiles/r06_config2_p256_counters.txt: 0.70 of one line per clock and
// CU).  Here a block serves one particle (or 1 / bpp of its angles): its waves copy the particle's byte image of the bounds
// (Slam2dLevel.gmin2b: cost >> 24, written beside gmin2; gp x lp bytes, 42 KB at config 2, three blocks per CU) into LDS, then wave w
// bounds its angles one after the other: lane = one pose tile (NSET tiles per lane), one ds_read_u8 per cell and tile set --
// 2 LDS cycles per wave instruction instead of ~20 L1 cycles.  The bound is looser by < 2^-7 per cell (floor of 12 more bits;
// 1.2 at 158 cells against the margin of 30): a few more tiles survive, the results do not change (every surviving tile is
// scored exactly).  Lists are padded to a multiple of BL_BATCH cells with the cell at offset 0; what the padding added is
// taken off afterwards.
// Seeds: as k_bound, the best-bound tile of an angle is scored exactly -- unless its bound does not exceed lv.bnb_best[p] any
// more (a wave's second and third angles mostly find it raised by the first round's seeds): a seed's exact score cannot exceed
// its bound, so the FINAL bnb_best is the maximum over all seeds whatever is skipped, in whatever order (k_bound2's rule).
#define BL_BATCH 16
#ifndef BL_RLE_BATCH
#define BL_RLE_BATCH 8       // (runs of a 64-cell chunk: ~22 at config 5 -- batches of 16 waste a third of their gathers)
#endif
// RLE (long lists: ~1000 beams): neighbouring beams end in the same 4 x 4-cell block more often than not, so a wave's 64 cell offsets are
// run-length compressed first (ballot of the run heads, the (offset, run length) pairs compacted through 256 bytes of LDS per wave)
// and the gathers go over the runs: sum += entry x run length.
//
// refresh != 0 (the host folded k_blur_check_redo's launch away: fold_field_check): the prologue also brings the bound minima up
// to date, which that launch did between the blur and this kernel.  What gmin2_dirty refreshes -- for every tile written at this
// build (the triage's blur list and fill list) 5 rows of 1 + 4 + 1 entries, entry = min(2 x 2 of gmin), border tiles entry by
// entry -- reads only the block minima of EARLIER launches (blur, triage fill), complete when this kernel starts: no barrier
// between a particle's blocks is needed.  Every block patches the entries' bytes (>> 24) into ITS OWN LDS image; the block with
// part == 0 also stores gmin2 (>> 12) and gmin2b to memory, the very values the separate launch left there -- a later scan
// stages the entries that are not dirty then from gmin2b, and the level may be bounded through the 32-bit gmin2 later on.
// Order: a dirty byte reaches LDS twice, stale with the staging copy and fresh with the refresh, so one barrier separates the
// staging stores (any wave's) from the refresh stores; the refresh's loads (tilecount -> list -> gmin rows) are issued BEFORE
// that barrier, beside the staging loads, so that only its stores lie behind it.  Sibling blocks of the particle may stage
// while block part == 0 rewrites the same bytes of gmin2b: they see the old or the new value of a byte and then overwrite
// exactly those bytes in LDS with the new one -- the image does not depend on the timing.
// A frame without a free tile (!min_known: rare; the blur's tail has checked its minimum and redone the clamp) gets the
// whole-frame pass of gmin2_pass instead -- its rows and columns are not those the tile lists reach.
enum { REFRESH_NONE = 0, REFRESH_ROW = 1, REFRESH_BORDER = 2 };
struct RefreshRow { int kind, Y, X0; Gmin2Row m; };
// one entry, the slow way: loads and stores (border tiles, the whole-frame pass)
__device__ __forceinline__ void bound_refresh_entry(const uint32_t* __restrict__ G, uint32_t* __restrict__ G2, uint8_t* __restrict__ G2B,
                                                    unsigned char* g2s, const int gp, const int lp, const int Y, const int X,
                                                    const bool writer) {
    const uint32_t v = gmin2_min2x2(G, gp, Y, X);
    g2s[Y * lp + X] = (unsigned char)(v >> 24);
    if (writer) {
        G2[(size_t)Y * gp + X] = v >> 12;
        G2B[(size_t)Y * lp + X] = (uint8_t)(v >> 24);
    }
}
// task idx = (tile idx / 5 of the two lists, entry row idx % 5): the tile, then the row's minima into registers (interior
// tiles; nothing is stored)
__device__ __forceinline__ int bound_refresh_tile(const int* __restrict__ list, const int ntile, const int nb, const int idx) {
    const int k = idx / 5;
    return k < nb ? list[k] : list[ntile + (k - nb)];
}
__device__ __forceinline__ RefreshRow bound_refresh_load(const uint32_t* __restrict__ G, const int tmax, const int gp, const int t, const int idx) {
    RefreshRow row{REFRESH_NONE, 0, 0, Gmin2Row{0u, gu4{0u, 0u, 0u, 0u}}};
    const int r = idx % 5;
    const int ty = t / tmax, tx = t - ty * tmax;
    const int Y = 4 * ty - 1 + r;
    if (Y < 0 || Y >= gp) return row;
    row.Y = Y; row.X0 = 4 * tx;
    if (gmin2_row_on_border(tmax, gp, tx, Y)) { row.kind = REFRESH_BORDER; return row; }
    row.m = gmin2_row_minima(G, gp, Y, tx);
    row.kind = REFRESH_ROW;
    return row;
}
__device__ __forceinline__ void bound_refresh_store(const RefreshRow& row, const uint32_t* __restrict__ G, uint32_t* __restrict__ G2,
                                                    uint8_t* __restrict__ G2B, unsigned char* g2s, const int gp, const int lp,
                                                    const bool writer) {
    if (row.kind == REFRESH_BORDER) {
        for (int c = 0; c < 5; ++c) {
            const int X = row.X0 - 1 + c;
            if (X >= 0 && X < gp) bound_refresh_entry(G, G2, G2B, g2s, gp, lp, row.Y, X, writer);
        }
        return;
    }
    if (row.kind != REFRESH_ROW) return;
    gmin2_row_store_bytes(row.m, g2s + row.Y * lp + row.X0);                  // (lp % 16 == 0, X0 % 4 == 0: an aligned word)
    if (writer) {
        gmin2_row_store_words(row.m, G2 + (size_t)row.Y * gp + row.X0);
        gmin2_row_store_bytes(row.m, G2B + (size_t)row.Y * lp + row.X0);
    }
}
// the whole frame, as gmin2_pass covers it (a frame without a free tile: once in a blue moon, may be slow)
__device__ __forceinline__ void bound_refresh_frame(const uint32_t* __restrict__ G, uint32_t* __restrict__ G2, uint8_t* __restrict__ G2B,
                                                 unsigned char* g2s, const int gp, const int lp, const int rows, const int cols,
                                                 const bool writer) {
    for (int idx = threadIdx.x; idx < rows * cols; idx += blockDim.x) {
        const int Y = idx / cols, X = idx - Y * cols;
        bound_refresh_entry(G, G2, G2B, g2s, gp, lp, Y, X, writer);
    }
}
//
// HOIST (short lists, NSET <= 2: the wider instantiations spill with it): what a wave's FIRST angle reads from the lists k_endpoints
// wrote -- kcount, its lane's entry of pcells, the head of cells that the seed's prefetch covers (BL_HEAD entries), and bnb_best --
// has addresses known at the kernel's first instruction, and each is a first touch of another kernel's data: a round trip of its
// own where it stood (behind the staging barrier, one after the other).  They are issued ahead of the staging loads instead and
// travel with the image.  Nothing waits for K: the rows of pcells and cells are kmax long, so the index is clamped to the row and
// the `k < K` masks are applied when K has arrived.  The list head waits in a slot of BL_HEAD words per wave behind the image
// (held in registers across the loop it spills); the seed reads it back as k_exact_select reads its staged lists.  bnb_best read
// early is an older value: by the rule above it can only let more seeds be scored, the final maximum is the same.  A wave's later
// angles (64 particles per launch and more) load as before.
#define BL_HEAD 256
template <int NSET, bool RLE, bool HOIST = false>
__global__ __launch_bounds__(1024) void k_bound_lds(Slam2dLevel lv, int P, int bpp, int tpb, int refresh) {
    static_assert(!HOIST || (!RLE && NSET <= 2), "the hoisted form exists for short lists and one or two tile sets");
    extern __shared__ __attribute__((aligned(16))) unsigned char g2s[];                  // [gp][lp] (+ RLE: [waves][64] words; HOIST: [waves][BL_HEAD] words)
    const int lp = lv.g2b_pitch;
    const int b = blockIdx.x;
    int p, part;
    xcd_particle(b, bpp, &p, &part);
    if (p >= P) return;
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, nw = blockDim.x >> 6;
    const int nbt = cube_of(lv).nbt, nbq4 = cube_of(lv).nbq4;
    const int gp = lv.tmax << 2;
    DBG_CLOCK(0, b == 0);
    // angles from the middle of the block's range outwards: the first round (which finds lv.bnb_best[p] at -inf and scores every
    // seed) then holds the angles nearest the estimate's, where a tracked pose has its maximum
    const int it0 = part * tpb, it_end = min(lv.ntheta, it0 + tpb);
    const int nth = it_end - it0, mid = (nth - 1) >> 1;
    auto angle_of = [&](const int j) -> int { return it0 + mid + ((j & 1) ? ((j + 1) >> 1) : -((j + 1) >> 1)); };
    int hK = 0, hcv = 0, hcl[BL_HEAD / WAVE] = {};
    unsigned long long hbest = 0ull;
    if constexpr (HOIST) {                                  // the first angle's loads (see above): in flight with the image
        if (w < nth && lv.kmax > 0) {
            const size_t row = (size_t)p * lv.ntheta + angle_of(w);
            const int* __restrict__ pcl = lv.pcells + row * lv.kmax;
            const int* __restrict__ cl = lv.cells + row * lv.kmax;
            hK = lv.kcount[row];
            hcv = pcl[min(lane, lv.kmax - 1)];
            hbest = __hip_atomic_load(&lv.bnb_best[p], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#pragma unroll
            for (int i = 0; i < BL_HEAD / WAVE; ++i) hcl[i] = cl[min(lane + WAVE * i, lv.kmax - 1)];
        }
    }
    // the refresh's chain starts ahead of the staging loads (refresh, and hence every branch on it, is uniform over the launch)
    // -- tile counts, then this thread's tile of the lists: in flight with the image
    const int ntile = lv.tmax * lv.tmax;
    const int* __restrict__ dlist = lv.tilelist + (size_t)p * 2 * ntile;
    int nblur = 0, ndirty = 0, min_known = 1, dtile = 0;
    if (refresh) {
        min_known = lv.frames[p].min_known;
        nblur = lv.tilecount[2 * p];
        ndirty = min_known ? (nblur + lv.tilecount[2 * p + 1]) * 5 : 0;
        if (tid < ndirty) dtile = bound_refresh_tile(dlist, ntile, nblur, tid);
    }
    {   // the image, as it lies in memory: 16-byte chunks, four loads in flight per thread
        const u32x4* __restrict__ src = reinterpret_cast<const u32x4*>(lv.gmin2b + (size_t)p * gp * lp);
        u32x4* dst = reinterpret_cast<u32x4*>(g2s);
        const int n16 = (gp * lp) >> 4, nt = blockDim.x;
        for (int i = tid; i < n16; i += 4 * nt) {
            u32x4 v[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) if (i + k * nt < n16) v[k] = src[i + k * nt];
#pragma unroll
            for (int k = 0; k < 4; ++k) if (i + k * nt < n16) dst[i + k * nt] = v[k];
        }
    }
    int* const head_s = reinterpret_cast<int*>(g2s + (((size_t)gp * lp + 15) & ~(size_t)15)) + w * BL_HEAD;      // (HOIST: this wave's slot)
    if constexpr (HOIST) {
#pragma unroll
        for (int i = 0; i < BL_HEAD / WAVE; ++i) head_s[lane + WAVE * i] = hcl[i];
    }
    DBG_CLOCK(1, b == 0);
    if (refresh) {                                          // the bound minima of the tiles written at this build (see above)
        const int nt = blockDim.x;
        const uint32_t* __restrict__ G = lv.gmin + (size_t)p * gp * gp;
        uint32_t* __restrict__ G2 = lv.gmin2 + (size_t)p * gp * gp;
        uint8_t* __restrict__ G2B = lv.gmin2b + (size_t)p * gp * lp;
        const bool writer = part == 0;
        RefreshRow row{REFRESH_NONE, 0, 0, Gmin2Row{0u, gu4{0u, 0u, 0u, 0u}}};
        if (tid < ndirty) row = bound_refresh_load(G, lv.tmax, gp, dtile, tid);                    // loads only
        __syncthreads();                                    // every wave's staging stores lie before any refresh store
        bound_refresh_store(row, G, G2, G2B, g2s, gp, lp, writer);
        for (int idx = tid + nt; idx < ndirty; idx += nt)   // (more tasks than threads: a launch of few waves, a long list)
            bound_refresh_store(bound_refresh_load(G, lv.tmax, gp, bound_refresh_tile(dlist, ntile, nblur, idx), idx), G, G2, G2B, g2s, gp, lp, writer);
        if (!min_known) {
            // (block-uniform; rare.)  Every block of the particle walks the whole frame, four dependent 4-byte loads and a byte
            // store per entry, ~30 000 entries over <= 1024 threads at config 2: some tens of microseconds, in a scan whose blur
            // has just redone every tile of the frame with one wave
            const Slam2dFrame fr = lv.frames[p];
            bound_refresh_frame(G, G2, G2B, g2s, gp, lp, min(gp, (fr.fh >> 2) + 2), min(gp, (fr.fw >> 2) + 2), writer);
        }
    }
    // this lane's tiles (byte offsets into the LDS image, slots of the bounds array)
    int lbase[NSET], tslot[NSET];
    bool valid[NSET];
#pragma unroll
    for (int s = 0; s < NSET; ++s) {
        const int t = s * WAVE + lane;
        valid[s] = t < nbt * nbt;
        const int by = valid[s] ? t / nbt : 0, bx = valid[s] ? t - by * nbt : 0;
        lbase[s] = by * lp + bx;
        tslot[s] = (by << 8) | bx;
    }
    const double inv = 1.0 / lv.cost_scale;
    const double* __restrict__ pm = lv.tile_pmax + (size_t)p * nbt * nbq4;
    double pmx[NSET];
#pragma unroll
    for (int s = 0; s < NSET; ++s) pmx[s] = valid[s] ? pm[(tslot[s] >> 8) * nbq4 + (tslot[s] & 255)] : -INFINITY;
    const unsigned magic = (unsigned)((0x100000000ull + (unsigned)gp - 1u) / (unsigned)gp);      // e / gp = umulhi(e, magic), e < 2^32 / gp
    __syncthreads();
    // (the hoisted values are first USED here: without this the compiler moves conv()'s shift up to the load and waits for it
    // in front of the staging loads)
    if constexpr (HOIST) asm volatile("" : "+v"(hK), "+v"(hcv));
    DBG_CLOCK(2, b == 0);
    double seedU = -INFINITY;
    int seedT = INT_MAX, seedIt = 0, seedK = 0;
    for (int j = w; j < nth; j += nw) {
        const int it = angle_of(j);
        const bool hoisted = HOIST && j == w && lv.kmax > 0;        // (wave-uniform)
        const int K = hoisted ? hK : lv.kcount[p * lv.ntheta + it];
        const int* __restrict__ pcl = lv.pcells + ((size_t)p * lv.ntheta + it) * lv.kmax;
        unsigned sum[NSET];
#pragma unroll
        for (int s = 0; s < NSET; ++s) sum[s] = 0u;
        // a cell's byte offset into gmin2 ((Y0 gp + X0) 4) -> into the LDS image (Y0 lp + X0); beyond the list: offset 0
        auto conv_of = [&](const int k, const int raw) -> int {
            if (k >= K) return 0;
            const unsigned e = (unsigned)raw >> 2, Y0 = __umulhi(e, magic);
            return (int)(Y0 * (unsigned)lp + (e - Y0 * (unsigned)gp));
        };
        auto conv = [&](const int k) -> int { return k >= K ? 0 : conv_of(k, pcl[k]); };
        int cv = hoisted ? conv_of(lane, hcv) : conv(lane);
        for (int base = 0; base < K; base += WAVE) {
            const int cur = cv;
            if (base + WAVE < K) cv = conv(base + WAVE + lane);
            if constexpr (RLE) {
                volatile unsigned* rl = reinterpret_cast<volatile unsigned*>(g2s + (((size_t)gp * lp + 15) & ~(size_t)15)) + w * WAVE;
                const int n = min(WAVE, K - base);
                const int prev = __shfl_up(cur, 1);
                const bool head = lane < n && (lane == 0 || cur != prev);
                const unsigned long long hm = __ballot(head);
                const unsigned long long below = lane ? (~0ull >> (64 - lane)) : 0ull;
                const int nu = __popcll(hm);
                if (head) {
                    const unsigned long long later = hm & ~(below | (1ull << lane));
                    const int nxt = later ? __ffsll((long long)later) - 1 : n;
                    rl[__popcll(hm & below)] = (unsigned)cur | ((unsigned)(nxt - lane) << 16);     // (offsets < 64 KB: checked at the launch)
                }
                const unsigned comp = lane < nu ? rl[lane] : 0u;                                    // (one wave: its LDS operations stay in order)
#pragma unroll
                for (int j0 = 0; j0 < WAVE; j0 += BL_RLE_BATCH) {
                    if (j0 < nu) {                              // (wave-uniform)
                        unsigned char v[NSET][BL_RLE_BATCH];
                        unsigned cnt[BL_RLE_BATCH];
#pragma unroll
                        for (int i = 0; i < BL_RLE_BATCH; ++i) {
                            const unsigned so = (unsigned)__builtin_amdgcn_readlane((int)comp, j0 + i);
                            cnt[i] = so >> 16;
#pragma unroll
                            for (int s = 0; s < NSET; ++s) v[s][i] = g2s[lbase[s] + (int)(so & 0xFFFFu)];
                        }
#pragma unroll
                        for (int i = 0; i < BL_RLE_BATCH; ++i)
#pragma unroll
                            for (int s = 0; s < NSET; ++s) sum[s] += (unsigned)v[s][i] * cnt[i];
                    }
                }
            } else {
#pragma unroll
            for (int j0 = 0; j0 < WAVE; j0 += BL_BATCH) {
                if (base + j0 < K) {                        // (wave-uniform)
                    unsigned char v[NSET][BL_BATCH];
#pragma unroll
                    for (int i = 0; i < BL_BATCH; ++i) {
                        const int so = __builtin_amdgcn_readlane(cur, j0 + i);
#pragma unroll
                        for (int s = 0; s < NSET; ++s) v[s][i] = g2s[lbase[s] + so];
                    }
#pragma unroll
                    for (int i = 0; i < BL_BATCH; ++i)
#pragma unroll
                        for (int s = 0; s < NSET; ++s) sum[s] += v[s][i];
                }
            }
            }
        }
        DBG_CLOCK(3, b == 0 && j == 0);
        const unsigned npad = RLE ? 0u : (unsigned)(((K + BL_BATCH - 1) / BL_BATCH) * BL_BATCH - K);
        double* __restrict__ bnd = lv.bounds + ((size_t)p * lv.ntheta + it) * nbt * nbq4;
        Best me{-INFINITY, INT_MAX, 0};
#pragma unroll
        for (int s = 0; s < NSET; ++s) {
            if (valid[s]) {
                const unsigned sm = sum[s] - npad * (unsigned)g2s[lbase[s]];
                // as k_bound: U >= every pose's score of the tile; L = (sum of the block minima >> 24) << 24
                const double U = (-(((double)sm * 16777216.0) * inv) + pmx[s]) + 1e-9;
                bnd[(tslot[s] >> 8) * nbq4 + (tslot[s] & 255)] = U;
                Best cand{U, tslot[s], 0};
                if (better(cand, me)) me = cand;
            }
        }
        if (lane < nbt)                                                     // padding tiles of every tile row: -inf
            for (int bx = nbt; bx < nbq4; ++bx) bnd[lane * nbq4 + bx] = -INFINITY;
        me = wave_best_fast(me);
        if (lv.theta_umax && lane == 0) lv.theta_umax[(size_t)p * lv.ntheta + it] = me.i != INT_MAX ? me.v : -INFINITY;
        DBG_CLOCK(4, b == 0 && j == 0);
        if (me.i == INT_MAX) continue;
        if (RLE) {
            // long lists: a seed costs as much as the angle's bounds (16 poses x ~1000 cells: 17.8 us against 16.0 at config 5), and the
            // looser byte bounds let few later seeds be skipped -- the wave scores ONE seed, that of its angle with the largest
            // bound (the particle's largest bound is some wave's largest: the seed that matters is among them)
            if (me.v > seedU || seedT == INT_MAX) { seedU = me.v; seedT = me.i; seedIt = it; seedK = K; }
            continue;
        }
        const unsigned long long best = hoisted ? hbest : __hip_atomic_load(&lv.bnb_best[p], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (!(me.v > unorder_bits(best))) continue;                         // (wave-uniform; bounds are never NaN: tile_pmax maps NaN to +inf)
        const int* __restrict__ cl = lv.cells + ((size_t)p * lv.ntheta + it) * lv.kmax;
        if constexpr (HOIST) {
            int pre[16];
            if (hoisted) {                                                  // tile_prefetch<16>, from the wave's slot
                const int sl = lane & 15;
#pragma unroll
                for (int i = 0; i < 16; ++i) pre[i] = sl + 16 * i < K ? head_s[sl + 16 * i] * 4 : 0x7ffffff0;
            } else {
                tile_prefetch<16>(cl, K, pre);
            }
            tile_seed<16>(lv, p, me.i >> 8, me.i & 255, cl, K, inv, pre);
        } else {
            bound_seed_exact(lv, p, me.i >> 8, me.i & 255, cl, K, inv);
        }
        DBG_CLOCK(5, b == 0 && j == 0);
    }
    if (RLE && seedT != INT_MAX) {
        const unsigned long long best = __hip_atomic_load(&lv.bnb_best[p], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (seedU > unorder_bits(best))
            bound_seed_exact(lv, p, seedT >> 8, seedT & 255, lv.cells + ((size_t)p * lv.ntheta + seedIt) * lv.kmax, seedK, inv);
    }
    DBG_CLOCK(14, b == 0);
}

// Two-level bounds for long cell lists (Slam2dLevel.bnb == 2; K ~ 1000 at 1081 beams, where k_bound sits at its
// texture-path bound of one load instruction per cell and theta).  Level 1: tiles of 8 x 8 poses, bounded through gmin3d
// (the 8 x 8 cell window of such a tile lies inside 3 x 3 aligned 4 x 4 blocks); a tile row is 2 quads, a cell 12-16 lanes,
// so ONE load instruction serves 4-5 cells.  Level 2 (k_bound2): the four 4 x 4-pose children of the few level-1 tiles that
// survive (0.3 per theta at config 5) get their gmin2 bound; every other 4 x 4 tile's bound is -inf.  k_exact_select is
// unchanged.  The seed: best level-1 tile -> its best child by level-2 bound -> exact.
// level-2 bounds of the four children of level-1 tile (R, Cx): lane = (child c = lane / 16, cell slice lane % 16); returns
// the child's bound in every lane of its row (-inf for a child outside the cube)
__device__ __forceinline__ double children_bounds(const Slam2dLevel& lv, const __amdgpu_buffer_rsrc_t rg2, const int* __restrict__ pcl,
                                                  const int K, const int R, const int Cx, const double* __restrict__ pm,
                                                  const int nbt, const int nbq4, const int gp, const double inv) {
    const int lane = threadIdx.x & 63, c = lane >> 4, sl = lane & 15;
    const int cy = 2 * R + (c >> 1), cx = 2 * Cx + (c & 1);
    const bool valid = cy < nbt && cx < nbt;
    const int lanepart = (cy * gp + cx) * 4;
    unsigned sum = 0u;
    for (int k = sl; k < K; k += 16 * 8) {
        int off[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) off[i] = (valid && k + 16 * i < K) ? lanepart + pcl[k + 16 * i] : 0x7ffffff0;
        unsigned v[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) v[i] = __builtin_amdgcn_raw_buffer_load_b32(rg2, off[i], 0, 0);
#pragma unroll
        for (int i = 0; i < 8; ++i) sum += v[i];
    }
    sum = row16_sum_u32(sum);
    return valid ? (-(((double)sum * 4096.0) * inv) + pm[cy * nbq4 + cx]) + 1e-9 : -INFINITY;
}

#define B1_DEPTH 16
__global__ __launch_bounds__(64) void k_bound1(Slam2dLevel lv, int P) {
    extern __shared__ __attribute__((aligned(16))) int b1_lds[];      // [64 * 4] partial sums, then [kmax] cell offsets
    int p, it;
    xcd_particle(blockIdx.x, lv.ntheta, &p, &it);
    if (p >= P) return;
    const int lane = threadIdx.x;
    const Cube cube = cube_of(lv);
    const int nx = cube.nx, nbt = cube.nbt, nbq4 = cube.nbq4;
    const int nb1 = (nx + 7) >> 3, nq1 = (nb1 + 3) >> 2, L = nb1 * nq1, C = WAVE / L;
    const int gp = lv.tmax << 2, hp = gp >> 1;
    const int K = lv.kcount[p * lv.ntheta + it];
    const int* __restrict__ p3 = lv.p3cells + ((size_t)p * lv.ntheta + it) * lv.kmax;
    unsigned* red = reinterpret_cast<unsigned*>(b1_lds);
    int* cs = b1_lds + WAVE * 4;
    for (int k = lane; k < K; k += WAVE) cs[k] = p3[k];
    const __amdgpu_buffer_rsrc_t rg3 = image_rsrc(lv.gmin3d + (size_t)p * gp * gp, (size_t)gp * gp * sizeof(uint32_t));
    const int g = lane / L, l2 = lane - g * L, r = l2 / nq1, q = l2 - r * nq1;
    const bool active = g < C;
    const int lanepart = (r * hp + 4 * q) * 4;
    unsigned sum[4] = {0u, 0u, 0u, 0u};
    __syncthreads();
    for (int k0 = 0; k0 < K; k0 += C * B1_DEPTH) {
        int off[B1_DEPTH];
#pragma unroll
        for (int i = 0; i < B1_DEPTH; ++i) {
            const int k = k0 + i * C + g;
            off[i] = (active && k < K) ? lanepart + cs[k] : 0x7ffffff0;
        }
        u32x4 v[B1_DEPTH];
#pragma unroll
        for (int i = 0; i < B1_DEPTH; ++i) v[i] = __builtin_amdgcn_raw_buffer_load_b128(rg3, off[i], 0, 0);
#pragma unroll
        for (int i = 0; i < B1_DEPTH; ++i)
#pragma unroll
            for (int e = 0; e < 4; ++e) sum[e] += v[i][e];
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) red[e * WAVE + lane] = sum[e];
    __syncthreads();
    const double inv = 1.0 / lv.cost_scale;
    const double* __restrict__ pm = lv.tile_pmax + (size_t)p * nbt * nbq4;
    double* __restrict__ b1 = lv.bounds1 + ((size_t)p * lv.ntheta + it) * 64;
    Best me{-INFINITY, INT_MAX, 0};
    if (lane < L) {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int c1 = 4 * q + e;
            if (c1 < 8) {
                unsigned tot = 0u;
                for (int g2 = 0; g2 < C; ++g2) tot += red[e * WAVE + g2 * L + lane];
                // largest prior of the tile's children (+inf if a child holds a NaN prior, -inf for a tile outside the cube)
                double pmx = -INFINITY;
                for (int a = 0; a < 2; ++a)
                    for (int bb = 0; bb < 2; ++bb)
                        if (2 * r + a < nbt && 2 * c1 + bb < nbt) pmx = fmax(pmx, pm[(2 * r + a) * nbq4 + 2 * c1 + bb]);
                const double U = (-(((double)tot * 4096.0) * inv) + pmx) + 1e-9;
                b1[r * 8 + c1] = U;
                Best cand{U, r * 8 + c1, 0};
                if (c1 < nb1 && better(cand, me)) me = cand;
            }
        }
    }
    if (lane >= L && lane < 64) {                           // level-1 tiles beyond the cube: never survive
        for (int t = lane - L; t < 64; t += 64 - L) {
            const int r1 = t >> 3, c1 = t & 7;
            if (r1 >= nb1 || c1 >= 4 * nq1) b1[t] = -INFINITY;
        }
    }
    me = wave_best_ordered(me);
    // candidate seed of the particle: its best finite level-1 bound over all theta (k_seed scores it exactly); the low
    // 14 bits of the bound make room for (theta, tile) -- this only picks WHERE the threshold is measured
    if (lane == 0 && me.v > -INFINITY && me.v < INFINITY)
        atomicMax(&lv.seed_key[p], (order_bits(me.v) & ~0x3FFFull) | (unsigned long long)((it << 6) | me.i));
}

// The threshold of a particle (bnb == 2): the level-1 tile with the best bound over all theta -> its best child by level-2
// bound -> that 4 x 4 tile exactly; the best of its 16 scores is a lower bound of the cube's maximum.  One block per
// particle, thread = cell (one seed per PARTICLE: the per-theta seeds of k_bound cost a third of its cache-line touches).
#define SEED_THREADS 1024
__global__ __launch_bounds__(SEED_THREADS) void k_seed(Slam2dLevel lv, int P) {
    __shared__ unsigned csum[4];
    __shared__ unsigned long long acc_s[16];
    __shared__ int best_s;
    const int p = blockIdx.x, tid = threadIdx.x;
    const unsigned long long key = lv.seed_key[p];
    if (!key) return;                                       // no finite bound anywhere: no threshold, every tile is scored
    const int it = (int)(key >> 6) & 0xFF, t1 = (int)key & 63, R = t1 >> 3, Cx = t1 & 7;
    const Cube cube = cube_of(lv);
    const int nx = cube.nx, npose = cube.npose, nbt = cube.nbt, nbq4 = cube.nbq4;
    const int gp = lv.tmax << 2;
    const int K = lv.kcount[p * lv.ntheta + it];
    const int* __restrict__ pcl = lv.pcells + ((size_t)p * lv.ntheta + it) * lv.kmax;
    const int* __restrict__ cl = lv.cells + ((size_t)p * lv.ntheta + it) * lv.kmax;
    if (tid < 4) csum[tid] = 0u;
    if (tid < 16) acc_s[tid] = 0ull;
    __syncthreads();
    {
        const __amdgpu_buffer_rsrc_t rg2 = image_rsrc(lv.gmin2 + (size_t)p * gp * gp, (size_t)gp * gp * sizeof(uint32_t));
        unsigned s4[4] = {0u, 0u, 0u, 0u};
        for (int k = tid; k < K; k += SEED_THREADS) {
            const int off = pcl[k];
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                const int cy = 2 * R + (c >> 1), cx = 2 * Cx + (c & 1);
                if (cy < nbt && cx < nbt) s4[c] += __builtin_amdgcn_raw_buffer_load_b32(rg2, (cy * gp + cx) * 4 + off, 0, 0);
            }
        }
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const unsigned t = row16_sum_u32(s4[c]);
            if ((tid & 15) == 0 && t) atomicAdd(&csum[c], t);
        }
    }
    __syncthreads();
    const double inv = 1.0 / lv.cost_scale;
    if (tid == 0) {
        const double* __restrict__ pm = lv.tile_pmax + (size_t)p * nbt * nbq4;
        int best = -1;
        double ub = -INFINITY;
        for (int c = 0; c < 4; ++c) {
            const int cy = 2 * R + (c >> 1), cx = 2 * Cx + (c & 1);
            if (cy >= nbt || cx >= nbt) continue;
            const double u = (-(((double)csum[c] * 4096.0) * inv) + pm[cy * nbq4 + cx]) + 1e-9;
            if (best < 0 || u > ub) { ub = u; best = c; }
        }
        best_s = best < 0 ? 0 : best;
    }
    __syncthreads();
    const int sby = 2 * R + (best_s >> 1), sbx = 2 * Cx + (best_s & 1);
    {
        const __amdgpu_buffer_rsrc_t rsrc = field_rsrc(lv, p);
        unsigned long long a[16];
#pragma unroll
        for (int i = 0; i < 16; ++i) a[i] = 0ull;
        for (int k = tid; k < K; k += SEED_THREADS) {
            const int off = cl[k] * 4;
            u32x4 v[4];
#pragma unroll
            for (int r = 0; r < 4; ++r) v[r] = __builtin_amdgcn_raw_buffer_load_b128(rsrc, ((4 * sby + r) * lv.fpitch + 4 * sbx) * 4 + off, 0, 0);
#pragma unroll
            for (int r = 0; r < 4; ++r)
#pragma unroll
                for (int e = 0; e < 4; ++e) a[r * 4 + e] += v[r][e];
        }
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const unsigned long long t = row16_sum_u64(a[i]);
            if ((tid & 15) == 0 && t) atomicAdd(&acc_s[i], t);
        }
    }
    __syncthreads();
    if (tid == 0) {
        const double* __restrict__ pr = lv.prior + (size_t)p * 2 * npose;
        double val = -INFINITY;
        for (int r = 0; r < 4; ++r)
            for (int e = 0; e < 4; ++e) {
                const int dy = 4 * sby + r, dx = 4 * sbx + e;
                if (dy >= nx || dx >= nx) continue;
                const double sc = pose_score(acc_s[r * 4 + e], inv, pr[dy * nx + dx], pr[npose + dy * nx + dx]);
                if (!isnan(sc)) val = fmax(val, sc);
            }
        if (val > -INFINITY) lv.bnb_best[p] = order_bits(val);
    }
}

// Level 2: the children of the level-1 tiles that reach the threshold get their gmin2 bounds (every other 4 x 4 tile: -inf);
// then the theta's best child is scored exactly when its bound still reaches the particle's best score, which tightens the
// threshold k_exact_select works with.  bnb_best rises while the kernel runs; the reads are racy on purpose: a tile or a
// seed that is skipped because of a fresher value has a bound below the FINAL best, so neither the final bnb_best (the
// maximum over all candidate seeds) nor the set of tiles k_exact_select keeps depends on the timing.
__global__ __launch_bounds__(64) void k_bound2(Slam2dLevel lv, int P) {
    int p, it;
    xcd_particle(blockIdx.x, lv.ntheta, &p, &it);
    if (p >= P) return;
    const int lane = threadIdx.x;
    const int nbt = cube_of(lv).nbt, nbq4 = cube_of(lv).nbq4, nt = nbt * nbq4;
    const int gp = lv.tmax << 2;
    const double thr = unorder_bits(__hip_atomic_load(&lv.bnb_best[p], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) - SLAM2D_BNB_MARGIN;
    double* __restrict__ bnd = lv.bounds + ((size_t)p * lv.ntheta + it) * nt;
    for (int t = lane; t < nt; t += WAVE) bnd[t] = -INFINITY;
    const double u1 = lv.bounds1[((size_t)p * lv.ntheta + it) * 64 + lane];
    unsigned long long todo = __ballot(u1 >= thr);
    if (!todo) return;
    const int K = lv.kcount[p * lv.ntheta + it];
    const int* __restrict__ pcl = lv.pcells + ((size_t)p * lv.ntheta + it) * lv.kmax;
    const int* __restrict__ cl = lv.cells + ((size_t)p * lv.ntheta + it) * lv.kmax;
    const double* __restrict__ pm = lv.tile_pmax + (size_t)p * nbt * nbq4;
    const __amdgpu_buffer_rsrc_t rg2 = image_rsrc(lv.gmin2 + (size_t)p * gp * gp, (size_t)gp * gp * sizeof(uint32_t));
    const double inv = 1.0 / lv.cost_scale;
    int pre[8];
    tile_prefetch<8>(cl, K, pre);                           // for the seed below
    double ub = -INFINITY;
    int seed = -1;
    while (todo) {
        const int t1 = __ffsll((long long)todo) - 1;
        todo &= todo - 1;
        const int R = t1 >> 3, Cx = t1 & 7;
        const double u2 = children_bounds(lv, rg2, pcl, K, R, Cx, pm, nbt, nbq4, gp, inv);
        const int c = lane >> 4, cy = 2 * R + (c >> 1), cx = 2 * Cx + (c & 1);
        if ((lane & 15) == 0 && cy < nbt && cx < nbt) bnd[cy * nbq4 + cx] = u2;
#pragma unroll
        for (int cc = 0; cc < 4; ++cc) {                    // (-inf for a child outside the cube)
            const double u = readlane_f64(u2, 16 * cc);
            if (u > ub) { ub = u; seed = (2 * R + (cc >> 1)) * nbq4 + 2 * Cx + (cc & 1); }
        }
    }
    if (seed < 0) return;
    if (ub < unorder_bits(__hip_atomic_load(&lv.bnb_best[p], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT))) return;
    tile_seed<8>(lv, p, seed / nbq4, seed % nbq4, cl, K, inv, pre);
}

// One block per particle: the tiles whose bound reaches bnb_best - SLAM2D_BNB_MARGIN, exactly, then the selection
// (np.argmax / np.random.choice / confidence, :133-143).  Everything serial in a single wave is slow here (an fp64
// exp is ~0.25 us when no other wave hides its latency, a vector-memory instruction costs the CU 16 clocks), so
// every stage is spread over the block and the tile loop issues as few memory instructions as it can:
//   scan     thread = consecutive (theta, tile) bounds; block-wide exclusive scan of the survivor counts -> an
//            ascending list of surviving tiles (= cube order of theta, then tile row, then tile column); meanwhile the
//            particle's cell lists are staged in LDS (when they fit)
//   tiles    one tile per wave, 16 waves at a time: lane = pose row x 1/16 of the cell list, 16-byte field loads,
//            DPP row sums; 16 lanes add the priors and store the scores (level->cube and LDS)
//   max      thread = scored pose -> block reduction -> the maximum M (np.argmax order: first NaN, else largest,
//            lowest index)
//   exp      thread = scored pose: exp(score - M) -> LDS; DPP row sums per tile; the first tile of every theta adds
//            up the theta's tiles
//   select   wave 0: cdf over theta, then over the pose rows of the chosen theta, then along the row
// More than XS_TILES surviving tiles (rare) are handled in passes; the row walk then re-reads the cube.
#define XS_THREADS 1024
#define XS_TILES 256
#define XS_MAX_PER 32
#define XS_CELLS 8192                // cell-list entries staged in LDS (ntheta * kmax: config 2 6480, reference 5400)
#define XS_SPLIT_MAX 8
#ifndef XS_SPLIT_STAGE_CELLS
#define XS_SPLIT_STAGE_CELLS 1       // split blocks stage all cell lists in LDS behind the scan (0: each tile's list from global memory)
#endif
#define XS_SPLIT_LIGHT 4             // blocks per particle that work when one list pass holds all surviving tiles
#define SLAM2D_BNB_MAX_THETA 256
// SPLIT: nsplit blocks per particle (all of them on the particle's XCD, for the field's sake).  Every block scans the
// particle's bounds (the same list comes out everywhere) and scores its share of the surviving tiles -- with one block
// per particle 64 of the 256 CUs worked and the particle with the most tiles (93 against a median of 27 at config 2) set
// the kernel's time.  The scores go to level->cube with write-through (sc1) stores; every wave drains its stores, the
// block takes a ticket from the particle's arrival counter (lv.sync: zero before the launch, put back to zero by the
// last arriver), and the block that draws the last ticket runs the rest -- maximum, exp, per-theta sums, selection -- over
// ALL the particle's tiles, reading the scores back with sc1 loads (MI355X_MICROARCH.md, "Inter-workgroup visibility":
// sc1 stores + a vmcnt(0) drain per storing wave + a relaxed agent-scope counter on the producer side, sc1 loads on the
// consumer side; nothing depends on where the blocks run).  The arithmetic of those stages and its order are the same
// as with one block, so the results are bit-identical whatever nsplit is.
__device__ __forceinline__ void store_score(double* dst, const double v, const bool through) {
    if (through) __hip_atomic_store(reinterpret_cast<unsigned long long*>(dst), (unsigned long long)__double_as_longlong(v), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    else *dst = v;
}
__device__ __forceinline__ double load_score(const double* src, const bool through) {
    if (through) return __longlong_as_double((long long)__hip_atomic_load(reinterpret_cast<const unsigned long long*>(src), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
    return *src;
}
template <bool SPLIT>
__global__ __launch_bounds__(XS_THREADS) void k_exact_select(Slam2dLevel lv, const double* __restrict__ est, int estride,
                                                             const double* __restrict__ uniform, Slam2dMatch* out, int P, int nsplit) {
    __shared__ int list_s[XS_TILES];                   // theta << 8 | tile, ascending
    __shared__ double sc_s[XS_TILES][16];              // a tile's scores (row-major 4 x 4, -inf = no pose), then exp(score - M)
    __shared__ double tsum_s[XS_TILES], tmax_s[XS_TILES];
    __shared__ int targ_s[XS_TILES], tnan_s[XS_TILES];
    __shared__ double S_s[SLAM2D_BNB_MAX_THETA];       // sum over the theta's scored poses of exp(score - M)
    __shared__ int kc_s[SLAM2D_BNB_MAX_THETA], j0_s[SLAM2D_BNB_MAX_THETA], jn_s[SLAM2D_BNB_MAX_THETA];
    __shared__ int cells_s[XS_CELLS];
    __shared__ int wtot_s[XS_THREADS / WAVE];
    __shared__ double wbv_s[XS_THREADS / WAVE];
    __shared__ int wbi_s[XS_THREADS / WAVE], wbn_s[XS_THREADS / WAVE];
    __shared__ double M_s[2];                          // [0] running maximum, [1] the one before this pass
    __shared__ int Mi_s[2];                            // its flat index, nan flag
    __shared__ int last_s;
    const int tid = threadIdx.x;
    int p = blockIdx.x, part = 0;
    if constexpr (SPLIT) {                             // block b runs on XCD b % 8: a particle's blocks share that XCD's L2
        xcd_particle(blockIdx.x, nsplit, &p, &part);
        if (p >= P) return;
    }
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63;
    const Cube cube = cube_of(lv);
    const int nx = cube.nx, npose = cube.npose, nbt = cube.nbt, nbq4 = cube.nbq4, nt = nbt * nbq4;
    const int ntot = lv.ntheta * nt;
    const double thr = unorder_bits(lv.bnb_best[p]) - SLAM2D_BNB_MARGIN;
    const double* __restrict__ bnd = lv.bounds + (size_t)p * ntot;
    // (what the selection tail needs from global memory is fetched now: a load there is a microsecond of one wave's serial chain)
    const double u_pre = uniform != nullptr ? uniform[p] : 0.0;
    const double th_pre = (tid & 63) < lv.ntheta ? lv.thetas[tid & 63] : 0.0;       // (lane i keeps angle i: the chosen one comes by v_readlane)
    const double ex = est[(size_t)p * estride], ey = est[(size_t)p * estride + 1], eth = est[(size_t)p * estride + 2];
    DBG_CLOCK(8, p == 0);
    // ---- scan ----
    const int per = (ntot + XS_THREADS - 1) / XS_THREADS;          // <= XS_MAX_PER (checked by the host)
    const int g0 = tid * per;
    unsigned keepbits = 0u;
    bool look = g0 < ntot;
    if (look && lv.theta_umax && lv.bnb == 1) {        // only the angles whose largest bound reaches the threshold can hold a surviving tile
        const double* __restrict__ um = lv.theta_umax + (size_t)p * lv.ntheta;
        look = false;
        for (int it = g0 / nt; it <= min(g0 + per - 1, ntot - 1) / nt; ++it) look |= um[it] >= thr;
    }
    if (look)
        for (int i = 0; i < per; ++i) {
            const int g = g0 + i;
            if (g < ntot && bnd[g] >= thr) keepbits |= 1u << i;    // (padding tiles hold -inf)
        }
    // (a block that scores a quarter of the tiles reads the few lists it needs from global memory instead of staging them all)
    const bool cells_in_lds = (!SPLIT || XS_SPLIT_STAGE_CELLS) && lv.ntheta * lv.kmax <= XS_CELLS;
    if (cells_in_lds) {
        const int* __restrict__ call = lv.cells + (size_t)p * lv.ntheta * lv.kmax;
        for (int i = tid; i < lv.ntheta * lv.kmax; i += XS_THREADS) cells_s[i] = call[i];
    }
    const int cnt = __popc(keepbits);
    const int incl = wave_scan_incl_i32(cnt);
    if (lane == WAVE - 1) wtot_s[wave] = incl;
    if (tid < lv.ntheta) { kc_s[tid] = lv.kcount[p * lv.ntheta + tid]; S_s[tid] = 0.0; }
    if (tid == 0) { M_s[0] = -INFINITY; Mi_s[0] = INT_MAX; Mi_s[1] = 0; }
    __syncthreads();
    int off = incl - cnt, n_all = 0;
    for (int w2 = 0; w2 < XS_THREADS / WAVE; ++w2) { const int c = wtot_s[w2]; if (w2 < wave) off += c; n_all += c; }
    DBG_CLOCK(9, p == 0);
    const __amdgpu_buffer_rsrc_t rsrc = field_rsrc(lv, p);
    const double* __restrict__ pr = lv.prior + (size_t)p * 2 * npose;
    const double inv = 1.0 / lv.cost_scale;
    // the pass's list: surviving tiles [base, base + XS_TILES) in ascending (theta, tile) order
    auto build_list = [&](const int base) {
        int o = off;
        for (int i = 0; i < per; ++i)
            if ((keepbits >> i) & 1u) {
                if (o >= base && o < base + XS_TILES) { const int g = g0 + i; list_s[o - base] = ((g / nt) << 8) | (g % nt); }
                ++o;
            }
    };
    // exact scores of the pass's tiles j = first, first + stride, ... (one tile per wave at a time): lane = pose row x 1/16
    // of the cell list, 16-byte field loads, DPP row sums; 16 lanes add the priors and store the scores
    auto score_tiles = [&](const int n, const int first, const int stride) {
        for (int j = first; j < n; j += stride) {
            const int ent = list_s[j];
            const int it = ent >> 8, t = ent & 255;
            const int by = t / nbq4, bx = t - by * nbq4;
            const int K = kc_s[it];
            const int* __restrict__ cl = lv.cells + ((size_t)p * lv.ntheta + it) * lv.kmax;
            int pre[12];
            if (cells_in_lds) {
                const int* cs = cells_s + it * lv.kmax;
                const int sl = lane & 15;
#pragma unroll
                for (int i = 0; i < 12; ++i) pre[i] = sl + 16 * i < K ? cs[sl + 16 * i] * 4 : 0x7ffffff0;
            } else {
                tile_prefetch<12>(cl, K, pre);
            }
            // the 16 scoring lanes (16 r + e: pose row r, column e of the tile) fetch their pose's priors now
            const int r = lane >> 4, e = lane & 15;
            const int dy = 4 * by + r, dx = 4 * bx + e;
            const bool scorer = e < 4 && dy < nx && dx < nx;
            const int qq = dy * nx + dx;
            double prv = 0.0, ptw = 0.0;
            if (scorer) { prv = pr[qq]; ptw = pr[npose + qq]; }
            unsigned long long acc[4];
            tile_exact<12>(lv, rsrc, cl, K, by, bx, pre, acc);
            double sc = -INFINITY;
            if (e < 4) {
                const unsigned long long a = e == 0 ? acc[0] : e == 1 ? acc[1] : e == 2 ? acc[2] : acc[3];
                if (scorer) {
                    sc = pose_score(a, inv, prv, ptw);
                    store_score(&lv.cube[((size_t)p * lv.ntheta + it) * npose + qq], sc, SPLIT);
                }
                if constexpr (!SPLIT) sc_s[j][r * 4 + e] = sc;
            }
            if constexpr (!SPLIT) {
                // the tile's maximum in np.argmax order (first NaN, else largest, lowest index): the scoring lanes 16 r + e
                // ascend with the flat pose index, so "lowest index" = lowest lane.  Quad butterflies, then the four rows.
                double mq = scorer && !isnan(sc) ? sc : -INFINITY;
                mq = fmax(mq, __longlong_as_double((long long)dpp_u64<0xB1>((unsigned long long)__double_as_longlong(mq))));
                mq = fmax(mq, __longlong_as_double((long long)dpp_u64<0x4E>((unsigned long long)__double_as_longlong(mq))));
                const double tmx = fmax(fmax(readlane_f64(mq, 0), readlane_f64(mq, 16)), fmax(readlane_f64(mq, 32), readlane_f64(mq, 48)));
                const unsigned long long nanm = __ballot(scorer && isnan(sc));
                const unsigned long long eqm = nanm ? nanm : __ballot(scorer && sc == tmx);
                if (lane == 0) {
                    int arg = INT_MAX;
                    if (eqm) {
                        const int l = __ffsll((long long)eqm) - 1;
                        arg = it * npose + (4 * by + (l >> 4)) * nx + 4 * bx + (l & 15);
                    }
                    tmax_s[j] = nanm ? NAN : tmx; targ_s[j] = arg; tnan_s[j] = nanm ? 1 : 0;
                }
            }
        }
    };
    if constexpr (SPLIT) {
        // Round 4: how many of the particle's blocks work depends on how many tiles survived.  The launch carries up to
        // XS_SPLIT_MAX blocks per particle; a particle with few surviving tiles (one list pass: the tracked case, 30-180 tiles)
        // keeps the four that measured best there, the others leave after their scan -- every block finds the same n_all, so
        // all agree on who stays and the ticket counts to that number.  A particle with many (a scan that does not fit its map:
        // hundreds to a thousand) uses all of them: k_exact_select 119 -> 92 us and 132 -> 92 us on the inputs of
        // bench.py's config2_displaced / config2_worst.  The scores and the order of every later stage do not depend on the
        // split, so results are the same bits either way.
        const int nsplit_all = nsplit;
        nsplit = n_all > XS_TILES ? nsplit_all : min(nsplit_all, XS_SPLIT_LIGHT);
        if (part >= nsplit) return;
        // ---- this block's share of the tiles, all passes; then the ticket ----
        for (int base = 0; base < n_all; base += XS_TILES) {           // (block-uniform)
            build_list(base);
            __syncthreads();
            score_tiles(min(XS_TILES, n_all - base), part + nsplit * wave, nsplit * (XS_THREADS / WAVE));
            __syncthreads();                                           // list_s is rebuilt by the next pass / the tail
        }
        // Publish / consume across blocks, the form MI355X_MICROARCH.md ("inter-workgroup visibility": valid forms) lists as "8-B agent
        // atomics both sides": the scores leave as relaxed agent-scope 8-byte atomic stores (global_store ... sc1: past this CU's L1,
        // the line dropped from the XCD's L2), every storing wave drains them (s_waitcnt vmcnt(0)), the block takes its ticket with an
        // agent-scope atomic, and the last block reads the scores back with relaxed agent-scope atomic loads (sc1: never served from
        // an L1).  No agent-scope fence on either side: a release (buffer_wbl2) costs 1.7-6.5 us per block and an acquire
        // (buffer_inv) 1.7 us (the guide's price list; round 2 measured this kernel at 134 us with them), and neither is needed when
        // both sides bypass the caches they would write back / invalidate.  What the C++ abstract machine is not told is kept in
        // order by the signal fences (compiler only) around the barrier.  tests/test_gpu_parity.py::test_split_exact_select_stress
        // runs 1 000 launches with every block count against the one-block path, bit for bit.
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");               // every storing wave drains its write-through stores
        __atomic_signal_fence(__ATOMIC_SEQ_CST);                       // (no instruction: the compiler may not move the score stores
        __syncthreads();                                               //  below the ticket, nor the read-back loads above it)
        if (tid == 0) {
            const unsigned ticket = __hip_atomic_fetch_add(&lv.sync[p * SLAM2D_SYNC_WORDS], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            const int last = ticket == (unsigned)(nsplit - 1);
            if (last) __hip_atomic_store(&lv.sync[p * SLAM2D_SYNC_WORDS], 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // ready for the next launch
            last_s = last;
        }
        __syncthreads();
        if (!last_s) return;
        __atomic_signal_fence(__ATOMIC_SEQ_CST);
    }
    int n = 0;
    for (int base = 0; base < n_all; base += XS_TILES) {           // (block-uniform)
        n = min(XS_TILES, n_all - base);
        if (!(SPLIT && n_all <= XS_TILES)) build_list(base);       // (a single pass: the list of the scoring phase is still there)
        if (tid < lv.ntheta) jn_s[tid] = 0;
        __syncthreads();
        DBG_CLOCK(10, p == 0 && base == 0);
        // ---- tiles ----
        if constexpr (!SPLIT) {
            score_tiles(n, wave, XS_THREADS / WAVE);
        } else {
            // every tile of the pass back from the cube (sc1 loads: the stores were write-through), then the tiles' maxima
            for (int i0 = 0; i0 < n * 16; i0 += XS_THREADS) {
                const int idx = i0 + tid;
                if (idx < n * 16) {
                    const int ent = list_s[idx >> 4], it = ent >> 8, t = ent & 255;
                    const int by = t / nbq4, bx = t - by * nbq4;
                    const int dy = 4 * by + ((idx >> 2) & 3), dx = 4 * bx + (idx & 3);
                    double sc = -INFINITY;
                    if (dy < nx && dx < nx) sc = load_score(&lv.cube[((size_t)p * lv.ntheta + it) * npose + dy * nx + dx], true);
                    sc_s[idx >> 4][idx & 15] = sc;
                }
            }
            __syncthreads();
            if (tid < n) {                                  // np.argmax order inside the tile: first NaN, else largest, lowest index
                const int ent = list_s[tid], it = ent >> 8, t = ent & 255;
                const int by = t / nbq4, bx = t - by * nbq4;
                double tmx = -INFINITY;
                int arg = INT_MAX, nan = 0;
                for (int i = 0; i < 16; ++i) {
                    const int dy = 4 * by + (i >> 2), dx = 4 * bx + (i & 3);
                    if (dy >= nx || dx >= nx) continue;
                    const double sc = sc_s[tid][i];
                    const int q = it * npose + dy * nx + dx;
                    if (isnan(sc)) { if (!nan) { nan = 1; arg = q; } }
                    else if (!nan && (arg == INT_MAX || sc > tmx)) { tmx = sc; arg = q; }
                }
                tmax_s[tid] = nan ? NAN : tmx; targ_s[tid] = arg; tnan_s[tid] = nan;
            }
        }
        __syncthreads();
        DBG_CLOCK(11, p == 0 && base == 0);
        // ---- maximum ----
        {
            if (wave < XS_TILES / WAVE) {                // thread = tile
                Best bme{-INFINITY, INT_MAX, 0};
                if (tid < n && targ_s[tid] != INT_MAX) bme = Best{tmax_s[tid], targ_s[tid], tnan_s[tid]};
                bme = wave_best_fast(bme);
                if (lane == 0) { wbv_s[wave] = bme.v; wbi_s[wave] = bme.i; wbn_s[wave] = bme.nan; }
            }
            __syncthreads();
            if (tid == 0) {
                Best rbest{M_s[0], Mi_s[0], Mi_s[1]};
                M_s[1] = M_s[0];
                for (int w2 = 0; w2 < XS_TILES / WAVE; ++w2) {
                    Best c{wbv_s[w2], wbi_s[w2], wbn_s[w2]};
                    if (c.i != INT_MAX && better(c, rbest)) rbest = c;
                }
                M_s[0] = rbest.v; Mi_s[0] = rbest.i; Mi_s[1] = rbest.nan;
            }
            __syncthreads();
        }
        const double M = M_s[0];
        DBG_CLOCK(29, p == 0 && base == 0);
        // ---- exp ----
        if (base > 0 && tid < lv.ntheta) S_s[tid] *= exp(M_s[1] - M);       // earlier passes: rescale to the new maximum
        for (int i0 = 0; i0 < n * 16; i0 += XS_THREADS) {                   // (block-uniform trip count)
            const int idx = i0 + tid;
            double ev = 0.0;
            if (idx < n * 16) {
                const double sc = sc_s[idx >> 4][idx & 15];
                ev = sc == -INFINITY ? 0.0 : exp(sc - M);
                sc_s[idx >> 4][idx & 15] = ev;
            }
            const unsigned long long tb = row16_sum_f64(ev);
            if (idx < n * 16 && (idx & 15) == 0) tsum_s[idx >> 4] = __longlong_as_double((long long)tb);
        }
        __syncthreads();
        DBG_CLOCK(30, p == 0 && base == 0);
        if (tid < n) {                                  // the first tile of a theta adds up the theta's tiles, in list order
            const int th = list_s[tid] >> 8;
            if (tid == 0 || (list_s[tid - 1] >> 8) != th) {
                double a = 0.0;
                int k = tid;
                for (; k < n && (list_s[k] >> 8) == th; ++k) a += tsum_s[k];
                S_s[th] += a;
                j0_s[th] = tid; jn_s[th] = k - tid;
            }
        }
        __syncthreads();
        DBG_CLOCK(12, p == 0 && base == 0);
    }
    if (wave != 0) return;
    // ---- selection (wave 0) ----
    const double M = M_s[0];
    const int nW = lv.ntheta;
    const int tper = (nW + WAVE - 1) / WAVE;
    const int w0 = lane * tper, w1 = min(nW, w0 + tper);
    double mine = 0.0;
    for (int w = w0; w < w1; ++w) mine += S_s[w];
    const double cinc = wave_scan_incl_f64(mine);
    const double total = readlane_f64(cinc, WAVE - 1);
    int pick = Mi_s[0];
    if (uniform != nullptr && !isnan(total)) {
        // np.random.choice(n, 1, p): first index whose normalised cdf exceeds u (:137-138); the poses that were not
        // scored carry < 1e-8 of the mass
        const double target = u_pre * total;
        const unsigned long long ahead = __ballot(cinc > target);
        const int lsel = ahead ? __ffsll((long long)ahead) - 1 : WAVE - 1;
        double run = readlane_f64(cinc - mine, lsel);
        const int s0 = min(lsel * tper, nW - 1), s1 = max(s0 + 1, min(nW, lsel * tper + tper));
        int it = s1 - 1;
        for (int w = s0; w < s1; ++w) {                           // wave-uniform loop
            const double t = S_s[w];
            if (run + t > target || w == s1 - 1) { it = w; break; }
            run += t;
        }
        while (it > 0 && !(S_s[it] > 0.0)) --it;                 // rounding fallback landed on a theta without a scored pose
        const int by = lane >> 2, rr = lane & 3;
        const bool in_lds = n_all <= XS_TILES;
        const int ja = in_lds ? j0_s[it] : 0, jb = in_lds ? ja + jn_s[it] : 0;
        double lsum = 0.0;
        bool has = false;
        if (in_lds) {
            // the theta's tiles are in LDS: lane = pose row dy, its poses in dx order (tiles ascend with bx)
            if (lane < nx)
                for (int j = ja; j < jb; ++j)
                    if ((list_s[j] & 255) / nbq4 == by) {
                        has = true;
#pragma unroll
                        for (int e = 0; e < 4; ++e) lsum += sc_s[j][rr * 4 + e];
                    }
        } else {
            const double* c = lv.cube + ((size_t)p * lv.ntheta + it) * npose;
            const double* bt = bnd + (size_t)it * nt;
            if (lane < nx)
                for (int bx = 0; bx < nbt; ++bx)
                    if (bt[by * nbq4 + bx] >= thr) {
                        has = true;
                        for (int e = 0; e < 4 && 4 * bx + e < nx; ++e) lsum += exp(load_score(&c[lane * nx + 4 * bx + e], SPLIT) - M);
                    }
        }
        const double linc = wave_scan_incl_f64(lsum);
        const unsigned long long hit = __ballot(has && run + linc > target);
        const unsigned long long have = __ballot(has);
        if (have) {
            const int l2 = hit ? __ffsll((long long)hit) - 1 : 63 - __clzll((long long)have);
            double r2 = run + readlane_f64(linc - lsum, l2);
            int found = -1, last = -1;
            if (lane == l2) {
                if (in_lds) {
                    for (int j = ja; j < jb && found < 0; ++j) {
                        const int t = list_s[j] & 255;
                        if (t / nbq4 == by) {
                            const int bx = t % nbq4;
                            for (int e = 0; e < 4 && 4 * bx + e < nx; ++e) {
                                last = it * npose + lane * nx + 4 * bx + e;
                                r2 += sc_s[j][rr * 4 + e];
                                if (r2 > target) { found = last; break; }
                            }
                        }
                    }
                } else {
                    const double* c = lv.cube + ((size_t)p * lv.ntheta + it) * npose;
                    const double* bt = bnd + (size_t)it * nt;
                    for (int bx = 0; bx < nbt && found < 0; ++bx)
                        if (bt[by * nbq4 + bx] >= thr)
                            for (int e = 0; e < 4 && 4 * bx + e < nx; ++e) {
                                last = it * npose + lane * nx + 4 * bx + e;
                                r2 += exp(load_score(&c[lane * nx + 4 * bx + e], SPLIT) - M);
                                if (r2 > target) { found = last; break; }
                            }
                }
                if (found < 0) found = last;                      // rounding fallback: the row's last scored pose
            }
            pick = __builtin_amdgcn_readlane(found, l2);
        }
    }
    const int it_sel = __builtin_amdgcn_readfirstlane(pick / npose);
    const double th_sel = lv.ntheta <= WAVE ? readlane_f64(th_pre, it_sel) : lv.thetas[it_sel];
    if (lane == 0) store_match(lv, p, ex, ey, eth, th_sel, pick, Mi_s[0], M, total, out);
    DBG_CLOCK(13, p == 0);
}

// ------------------------------------------------------------------------------------
// K4  weights                                        (Algorithm/FastSlam.py:30-48,135)
// ------------------------------------------------------------------------------------
// One 256-thread block.  `exchange`: the block runs beside the update blocks of the same launch (slam2d_scan_commit,
// slam2d_grid_update_weights), which may still raise bits: they are taken with an atomic exchange, so a bit raised
// after it stays in flags and is reported with the next scan instead of being lost.
// updateEstimatedPose of one particle (Algorithm/FastSlam.py:77-106): estimate = previous matched pose turned by the raw odometry's
// rotation; cos / sin of the expected moving direction (NaN: no direction known)
__device__ __forceinline__ void prior_one(const double* prev, const double* heading, const int p, const double raw_theta,
                                          const double prev_raw_theta, const int has_turn, const double raw_turn, double* est, double* psi_cs) {
    est[3 * p + 0] = prev[3 * p + 0];                                               // :79
    est[3 * p + 1] = prev[3 * p + 1];
    est[3 * p + 2] = prev[3 * p + 2] + raw_theta - prev_raw_theta;                  // :78
    double c = NAN, s = NAN;
    const double h = heading[p];
    if (has_turn && !isnan(h)) {                                                    // :89-95
        const double psi = h + raw_turn;
        c = cos(psi); s = sin(psi);
    }
    psi_cs[2 * p] = c; psi_cs[2 * p + 1] = s;
}
struct WeightsJob {
    double* logw; const double* logconf; int cstride; int N; double* w; double* stats; uint32_t* flags; uint32_t* flag_snapshot;
    // slam2d_scan_commit: the same block first does the scan's bookkeeping (k_post_match's work) for all particles
    const Slam2dMatch* fine; const Slam2dMatch* coarse; double* prev; double* heading; double* report;
    double* part;            // sharded filters: only the rank-local half (k_weights_local's work), the collective follows
    uint32_t abort_mask;     // slam2d_scan_commit: fault bits of the match that make the WHOLE launch a no-op (see there)
    const uint32_t* abort_flags; int abort_n;   // slam2d_groups_commit: the abort is decided over the fault bits of ALL groups (NULL: flags[0 .. N))
    // slam2d_scan_commit_next: the NEXT scan's pose prior (k_prior's work) behind this scan's bookkeeping, same thread per particle
    double* next_est; double* next_psi; double next_raw_theta, next_prev_raw_theta, next_raw_turn; int next_has_turn;
    // slam2d_groups_* with Slam2dScan.d_norm_sync (round 5): the groups' normaliser blocks merge among themselves on the device --
    // no stream, no event between the groups (normaliser_wait / normaliser_arrive)
    uint32_t* nsync = nullptr; int ngroups = 0, gidx = 0;
    const double* parts_all = nullptr; double* logw_all = nullptr; int n_all = 0; double total = 0.0; double* w_all = nullptr; double* stats_all = nullptr;
    // the scan's report pushed to the host by the block that finishes it (Slam2dScan.h_pack / h_seq, ABI 16): no copy, no event
    const double* pack_d = nullptr; double* pack_h = nullptr; int pack_n = 0; uint32_t* h_seq = nullptr; uint32_t seq = 0u;
    // the NEXT scan's ranges pulled from pinned host memory by the bookkeeping block, beside its prior (Slam2dScan.h_next_ranges)
    const double* pull_src = nullptr; double* pull_dst = nullptr; int pull_n = 0;
};
// Whoever finishes a scan for all groups -- the block that merged the normaliser, or the last group's block 0 of a voided scan --
// copies the scan's pack (report, weights, variance, fault-bit snapshot: device memory the groups' blocks have written and
// released) into the caller's pinned host buffer and publishes the scan's sequence number behind it, system scope: the host
// polls that word (slam2d_host_wait_seq) instead of waiting for a copy engine and an event (~15 us per scan).
__device__ __forceinline__ void publish_pack(const WeightsJob& wj) {
    if (!wj.h_seq) return;
    __syncthreads();
    for (int i = threadIdx.x; i < wj.pack_n; i += blockDim.x) wj.pack_h[i] = wj.pack_d[i];
    __threadfence_system();
    __syncthreads();
    if (threadIdx.x == 0) __hip_atomic_store(wj.h_seq, wj.seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
}
// pose / heading / log-weight bookkeeping of one particle after its match (Algorithm/FastSlam.py:110-117,134-135)
__device__ __forceinline__ void post_match_one(const Slam2dMatch* __restrict__ fine, const Slam2dMatch* __restrict__ coarse, const int p,
                                               double* prev, double* heading, double* logw, double* report) {
    const double x = fine[p].x, y = fine[p].y;
    const double mx = x - prev[3 * p], my = y - prev[3 * p + 1];                    // :110-111
    const double move = sqrt(mx * mx + my * my);
    double h = NAN;
    if (move != 0.0) h = my > 0.0 ? acos(mx / move) : -acos(mx / move);             // :113-117
    heading[p] = h;
    prev[3 * p] = x; prev[3 * p + 1] = y; prev[3 * p + 2] = fine[p].theta;          // :134
    logw[p] += coarse[p].log_confidence;                                            // :135
    if (report) {                                      // what the caller downloads once per scan
        report[5 * p] = x; report[5 * p + 1] = y; report[5 * p + 2] = fine[p].theta;
        report[5 * p + 3] = coarse[p].confidence; report[5 * p + 4] = coarse[p].log_confidence;       // :79 (coarse)
    }
}
__device__ __forceinline__ void weights_body(double* logw, const double* __restrict__ logconf, const int cstride, const int N,
                                             double* w, double* stats, uint32_t* flags, uint32_t* flag_snapshot, const bool exchange) {
    __shared__ double red[256];
    const int tid = threadIdx.x;
    if (flags)                                         // slam2d_scan_commit: the scan's fault bits move into the report
        for (int i = tid; i < N; i += 256) {
            if (exchange) flag_snapshot[i] = atomicExch(&flags[i], 0u);
            else { flag_snapshot[i] = flags[i]; flags[i] = 0u; }
        }
    double mx = -INFINITY;
    for (int i = tid; i < N; i += 256) {
        double v = logw[i] + (logconf ? logconf[(size_t)i * cstride] : 0.0);
        logw[i] = v;
        mx = fmax(mx, v);
    }
    red[tid] = mx;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) { if (tid < o) red[tid] = fmax(red[tid], red[tid + o]); __syncthreads(); }
    mx = red[0];
    __syncthreads();
    double s = 0.0;
    for (int i = tid; i < N; i += 256) s += exp(logw[i] - mx);
    red[tid] = s;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) { if (tid < o) red[tid] += red[tid + o]; __syncthreads(); }
    const double total = red[0];
    __syncthreads();
    const double lse = mx + log(total);
    double var = 0.0;
    for (int i = tid; i < N; i += 256) {
        const double wi = exp(logw[i] - mx) / total;                                 // :47-48
        w[i] = wi;
        logw[i] = logw[i] - lse;
        const double d = wi - 1.0 / (double)N;                                       // :34
        var += d * d;
    }
    red[tid] = var;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) { if (tid < o) red[tid] += red[tid + o]; __syncthreads(); }
    if (tid == 0) { stats[0] = red[0]; stats[1] = lse; }
}
// Sharded normaliser, rank-local half: log-weights += log-confidence, then this rank's
// [max log w, sum exp(lw - max), sum exp(2 (lw - max))].  The three doubles of every rank are
// exchanged by ONE all-gather (24 bytes per rank) and merged by k_weights_merge.
__device__ __forceinline__ void weights_local_body(double* logw, const double* __restrict__ logconf, const int cstride,
                                                   const int N, double* part) {
    __shared__ double red[256];
    __shared__ double red2[256];
    const int tid = threadIdx.x;
    double mx = -INFINITY;
    for (int i = tid; i < N; i += 256) {
        double v = logw[i] + (logconf ? logconf[(size_t)i * cstride] : 0.0);
        logw[i] = v;
        mx = fmax(mx, v);
    }
    red[tid] = mx;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) { if (tid < o) red[tid] = fmax(red[tid], red[tid + o]); __syncthreads(); }
    mx = red[0];
    __syncthreads();
    // A log-weight of -inf is weight 0 whatever the shard's maximum: with every entry -inf, exp(-inf - (-inf)) would be NaN, the
    // merges' NaN * exp(-inf - gm) = NaN * 0 too, and every rank's weights with it -- k_weights gives those particles 0 as long as
    // one particle anywhere is finite.  Such a shard leaves [-inf, 0, 0], the empty partial: the merges add 0 * 0.  A NaN entry is
    // not -inf: it still reaches the sums (fmax drops it from the maximum), and -inf everywhere is still NaN after the merges (their scale is
    // exp(-inf - (-inf)) then), like k_weights' 0 / 0.
    double s1 = 0.0, s2 = 0.0;
    for (int i = tid; i < N; i += 256) {
        const double v = logw[i];
        const double e = v == -INFINITY ? 0.0 : exp(v - mx);
        s1 += e;
        s2 += e * e;
    }
    red[tid] = s1;
    red2[tid] = s2;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (tid < o) { red[tid] += red[tid + o]; red2[tid] += red2[tid + o]; }
        __syncthreads();
    }
    if (tid == 0) { part[0] = mx; part[1] = red[0]; part[2] = red2[0]; }
}
__global__ __launch_bounds__(256) void k_weights_local(double* logw, const double* __restrict__ logconf, int cstride,
                                                       int N, double* part) {
    weights_local_body(logw, logconf, cstride, N, part);
}

// The normaliser of G particle groups WITHOUT a stream of its own (round 5).  Every group's map-update launch has one block that
// folds the scan's confidences into the group's log-weights and leaves the group's partial [max, sum, sum of squares]
// (weights_local_body); the merge over the groups (k_weights_merge's arithmetic, partials in group order: the same bits) used to be a
// launch on a third stream behind an event of every group, and every group's next update waited for an event behind it: two event
// packets between a group's kernels per scan, 6-8 us each on the group's own chain (kernel trace: exact -> update 6.5 us,
// update -> next endpoints 7.5 us of a 126 us step).  Now the blocks settle it among themselves through three kinds of device
// words (Slam2dScan.d_norm_sync, zeroed once): [0] arrivals of this scan, [1] merges completed so far, [2 + g] merges group g's next
// normaliser block has to see.  The block that arrives last merges for all groups and publishes; a group's next block waits for
// that before it touches its log-weights.  Plain stores + release fence before every flag, one acquire fence behind every wait
// (MI355X_MICROARCH.md, "inter-workgroup visibility", the valid producer / consumer forms): placement-independent.  No deadlock:
// a waiting block was enqueued after everything it waits for (slam2d_groups_* issue a whole scan of every group per call).
// All waits are BOUNDED: a producer that never comes -- a dead rank behind the all-gather, a caller that broke the
// whole-scan-per-call order -- ends as the fatal SLAM2D_F_SYNC_TIMEOUT in the group's fault words (word 62 of the sync block
// carries it from the gate kernel), not as a hung GPU.  The bound is word 59 of the sync block in milliseconds (0: 30 s -- round 5's
// fixed 2 s turned ordinary lateness into a fault: a peer rank behind the all-gather that grows its maps, a second process or a
// profiler on the GPU); slam2d_host_wait_seq's bound on the host side should exceed it.
#define SLAM2D_SYNC_DEFAULT_MS 30000u
__device__ __forceinline__ unsigned long long sync_spin_ticks(const uint32_t* nsync) {
    const uint32_t ms = __hip_atomic_load(&nsync[59], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    return (unsigned long long)(ms ? ms : SLAM2D_SYNC_DEFAULT_MS) * 100000ull;                 // (100 MHz wall clock)
}
__device__ __forceinline__ void normaliser_wait(uint32_t* nsync, const int g, uint32_t* flags) {
    if (threadIdx.x == 0) {
        const uint32_t want = nsync[2 + g];
        const unsigned long long t0 = wall_clock64(), SYNC_SPIN_TICKS = sync_spin_ticks(nsync);
        bool late = false;
        while ((int)(__hip_atomic_load(&nsync[1], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) - want) < 0) {
            __builtin_amdgcn_s_sleep(8);
            if (wall_clock64() - t0 > SYNC_SPIN_TICKS) { late = true; break; }
        }
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
        if ((late || __hip_atomic_load(&nsync[62], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) && flags) atomicOr(&flags[0], SLAM2D_F_SYNC_TIMEOUT);
    }
    __syncthreads();
}
__device__ __forceinline__ void normaliser_arrive(const WeightsJob& wj) {
    __shared__ int last_s;
    __syncthreads();                                       // every wave's stores of this block (log-weights, the partial) are out
    if (threadIdx.x == 0) {
        wj.nsync[2 + wj.gidx] += 1u;                       // (this group's next block: after THIS scan's merge)
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
        const uint32_t ticket = __hip_atomic_fetch_add(&wj.nsync[0], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        // (sharded, wj.logw_all == NULL: nobody merges here -- the caller's gate kernel on the normaliser's stream counts the arrivals,
        // the all-gather and slam2d_weights_merge_publish follow there)
        const int last = wj.logw_all != nullptr && ticket == (uint32_t)(wj.ngroups - 1);
        if (last) {
            __hip_atomic_store(&wj.nsync[0], 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);      // (nobody arrives for the next scan before the merge below is published)
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");                                      // the other groups' partials and log-weights
        }
        last_s = last;
    }
    __syncthreads();
    if (!last_s) return;
    // k_weights_merge's arithmetic, over the partials in group order
    const double* parts = wj.parts_all;
    double gm = -INFINITY;
    for (int r = 0; r < wj.ngroups; ++r) gm = fmax(gm, parts[3 * r]);
    double s1 = 0.0, s2 = 0.0;
    for (int r = 0; r < wj.ngroups; ++r) {
        const double sc = exp(parts[3 * r] - gm);
        s1 += parts[3 * r + 1] * sc;
        s2 += parts[3 * r + 2] * sc * sc;
    }
    const double lse = gm + log(s1);
    for (int i = threadIdx.x; i < wj.n_all; i += 256) {
        const double lw = wj.logw_all[i];
        wj.w_all[i] = exp(lw - gm) / s1;
        wj.logw_all[i] = lw - lse;
    }
    if (threadIdx.x == 0) { wj.stats_all[0] = s2 / (s1 * s1) - 1.0 / wj.total; wj.stats_all[1] = lse; }
    __syncthreads();
    if (threadIdx.x == 0) {
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
        const uint32_t gen = __hip_atomic_load(&wj.nsync[1], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(&wj.nsync[1], gen + 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    publish_pack(wj);                                      // (behind the word the groups wait for: the host is not on their path)
}
// A voided scan (k_grid_update's abort) has no normaliser: the groups' blocks 0 count themselves in word 60 instead and the last one
// publishes the report (fault-bit snapshot + coarse poses) to the host.
__device__ __forceinline__ void abort_arrive(const WeightsJob& wj) {
    if (!wj.h_seq || !wj.nsync) return;
    __shared__ int last_a;
    __syncthreads();
    if (threadIdx.x == 0) {
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
        const uint32_t ticket = __hip_atomic_fetch_add(&wj.nsync[60], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        const int last = ticket == (uint32_t)(wj.ngroups - 1);
        if (last) {
            __hip_atomic_store(&wj.nsync[60], 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
        }
        last_a = last;
    }
    __syncthreads();
    if (last_a) publish_pack(wj);
}

__global__ __launch_bounds__(256) void k_weights(double* logw, const double* __restrict__ logconf, int cstride, int N,
                                                 double* w, double* stats, uint32_t* flags, uint32_t* flag_snapshot) {
    weights_body(logw, logconf, cstride, N, w, stats, flags, flag_snapshot, false);
}

// ------------------------------------------------------------------------------------
// K3  occupancy-grid update                         (Utils/OccupancyGrid.py:127-152)
// ------------------------------------------------------------------------------------
// Beam-major update: the reference's own formulation (:134-152 walks the cells of each beam's spoke).
// Every spoke's cell list is ordered by radial band (SLAM2D_SPOKE_BAND cells of integer radius
// floor(r / unit) per band) and row-major inside a band, with the start of every band tabulated:
// a beam touches the bands up to the one holding range + w/2 -- work ~ touched cells (8 % of the
// W x W window on the Intel log) instead of the whole window -- and consecutive lanes fall on
// consecutive cells of a map row (the band is a short piece of the beam's wedge).  One wave per
// beam; a block takes UPDB_BEAMS adjacent beams of one particle (adjacent wedges share cache lines)
// and all blocks of a particle run on one XCD (block b -> XCD b % 8) so those lines meet in one L2.
// Each window cell belongs to exactly one spoke and each spoke to at most one beam: plain RMW.
#define UPDB_BEAMS 4                 // = waves per block
#ifndef UPDB_UNROLL
#define UPDB_UNROLL 4
#endif
#ifndef UPDB_NO_LATTICE
#define UPDB_NO_LATTICE 0            // 1: always the per-cell fp64 index path (A/B builds)
#endif
#ifndef UPDB_MIN_WAVES
#define UPDB_MIN_WAVES 1
#endif
#ifndef UPDB_SKIP_R
#define UPDB_SKIP_R 1
#endif

// ---- the spoke walk shared by k_grid_update, k_occ_extent, k_map_scans and k_predict_scan ----
// The spoke of a beam: spokesOffsetIdxByTheta = int(rint(theta / (2*pi) * numSpokes)) (:131) past the spoke of beam 0 (:134), in [0, S)
__device__ __forceinline__ int beam_spoke(const Slam2dLidar& lid, double th, int beam) {
    const int S = lid.num_spokes;
    int first = (lid.spoke_start + (int)rint(th / (2 * 3.141592653589793) * (double)S)) % S;
    if (first < 0) first += S;
    return (first + beam) % S;
}

// The tabulated band starts of a spoke's cell list: num_bands + 1 entries, the last one the list's end
__device__ __forceinline__ const int* spoke_bands(const Slam2dLidar& lid, const int spoke) {
    return lid.spoke_band + (size_t)spoke * (lid.num_bands + 1);
}

// The span [kbeg, kend) of a spoke's cell list that holds every cell with lo < r < hi, and kwall, the start of the band of lo.
// floor(r / unit) is monotone in r: cells with r > lo sit in bands >= band(lo), cells with r < hi in bands <= band(hi).  The
// cells of the bands wholly below band(lo) -- [kbeg, kwall) of a walk from the centre, which also wants the cells below lo (the
// free cells of a returned beam, :138) -- have floor(r / unit) < floor(lo / unit), hence r < lo, whatever the table says.
// false: hi admits no cell.
__device__ __forceinline__ bool beam_bands(const Slam2dLidar& lid, const int spoke, const double lo, const double hi, const bool from_centre,
                                           int& kbeg, int& kwall, int& kend) {
    const int nb = lid.num_bands;
    const int* __restrict__ bp = spoke_bands(lid, spoke);
    const int qlo = lo > 0.0 ? (int)fmin(floor(lo / lid.unit), 2.0e9) : 0;
    const int qhi = hi > 0.0 ? (int)fmin(floor(hi / lid.unit), 2.0e9) : -1;
    if (qhi < 0) return false;
    const int bw = min(qlo / SLAM2D_SPOKE_BAND, nb), b0 = from_centre ? 0 : bw, b1 = min(qhi / SLAM2D_SPOKE_BAND + 1, nb);
    kwall = bp[bw]; kbeg = bp[b0]; kend = bp[max(b0, b1)];
    return true;
}

// Window coordinate of column (row) j: np.linspace(-R, R, W)[j] = j * step + (-R), last element R (lut_xs_step, checked against
// the table by the host), else the table itself
__device__ __forceinline__ double window_coord(const Slam2dLidar& lid, const int j) {
    if (lid.lut_xs_step != 0.0) return j == lid.lut_w - 1 ? lid.max_range : (double)j * lid.lut_xs_step + -lid.max_range;
    return lid.lut_xs[j];
}

// The map index of a window cell is rint(((pose + xs[j]) - mapLim0) / unit) (:104-105,144-145), two fp64 chains per cell.  When
// the window step IS the map unit (lidarMaxRange a whole number of cells: every configuration in use) that is rint(A + j) with
// A = (pose - R - mapLim0) / unit: the fp64 evaluation differs from the real A + j by < 1e-11 cells (three roundings at magnitude
// <= 1e4), so it rounds to j + rint(A) whenever A is farther than 1e-6 from a half-integer -- decided once per wave: {on, rint(A)}.
// A pose that close to a rounding boundary, off the lattice or not finite is not `on` and takes window_map_index's per-cell path.
// (Config 5: 138 k waves x ~25 fp64 instructions per cell saved; the update is instruction-bound there.)
struct WindowLattice { bool on; int bx, by; };
__device__ __forceinline__ WindowLattice window_lattice(const Slam2dLidar& lid, const Slam2dMap& m, const double px, const double py,
                                                        const double inv_unit) {
    const double Ax = ((px + -lid.max_range) - m.lim_x0) * inv_unit, Ay = ((py + -lid.max_range) - m.lim_y0) * inv_unit;
    const double rAx = rint(Ax), rAy = rint(Ay);
    const bool on = lid.lut_xs_step == lid.unit && fabs(Ax) < 1e8 && fabs(Ay) < 1e8 &&
                    fabs(fabs(Ax - rAx) - 0.5) > 1e-6 && fabs(fabs(Ay - rAy) - 0.5) > 1e-6;
    return {on, on ? (int)rAx : 0, on ? (int)rAy : 0};
}

// convertRealXYToMapIdx (:104-105,144-145) of U window cells (row << 16 | column) of one lane: the integers of the exact division.
// Straight-line phases with no branch that depends on a lane.  On the lattice: column index + the wave's offset, nothing else.
// Off it, (int)rint(v / unit) without the fp64 division (~70 issue slots on gfx950, two per cell): v * (1 / unit) differs from
// v / unit by < 4e-16 relative, so the two round to the same integer unless the quotient is within 1e-6 of a half-integer --
// there, for the whole wave, the exact division decides.  A quotient that is NaN or not below 1e9 never reaches an integer
// conversion: its index is WINDOW_IDX_NONE, outside every map, and -- unlike -1, which Python's wrap sends to the last column --
// still negative after a stale-index launch's wrap and shifts (k_grid_update: - sx - ax + wc + ax, a map's rows * pitch < 2^32).
#define WINDOW_IDX_NONE (-(1 << 30))
template <int U>
__device__ __forceinline__ void window_map_index(const Slam2dLidar& lid, const Slam2dMap& m, const double px, const double py,
                                                 const double inv_unit, const bool lattice, const int bx, const int by,
                                                 const uint32_t (&cell)[U], int (&mxs)[U], int (&mys)[U]) {
    if (lattice) {                                             // (wave-uniform)
#pragma unroll
        for (int u = 0; u < U; ++u) {
            mxs[u] = (int)(cell[u] & 0xffffu) + bx;
            mys[u] = (int)(cell[u] >> 16) + by;
        }
        return;
    }
    double xj[U], yi[U];
    // (window_coord's own wave-uniform test, taken once ahead of the phase instead of between its loads: both arms are the same call)
    if (lid.lut_xs_step != 0.0) {
#pragma unroll
        for (int u = 0; u < U; ++u) {
            xj[u] = window_coord(lid, (int)(cell[u] & 0xffffu));
            yi[u] = window_coord(lid, (int)(cell[u] >> 16));
        }
    } else {
#pragma unroll
        for (int u = 0; u < U; ++u) {
            xj[u] = window_coord(lid, (int)(cell[u] & 0xffffu));
            yi[u] = window_coord(lid, (int)(cell[u] >> 16));
        }
    }
    bool slow = false;
#pragma unroll
    for (int u = 0; u < U; ++u) {
        const double tx = ((px + xj[u]) - m.lim_x0) * inv_unit, ty = ((py + yi[u]) - m.lim_y0) * inv_unit;
        const double rx = rint(tx), ry = rint(ty);
        slow |= fabs(fabs(tx - rx) - 0.5) < 1e-6 || fabs(fabs(ty - ry) - 0.5) < 1e-6 || !(fabs(tx) < 1e9) || !(fabs(ty) < 1e9);
        mxs[u] = (int)rx; mys[u] = (int)ry;                    // (a quotient beyond 1e9 is replaced below before anything reads this)
    }
    if (__any(slow)) {
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const double tx = ((px + xj[u]) - m.lim_x0) / lid.unit, ty = ((py + yi[u]) - m.lim_y0) / lid.unit;
            mxs[u] = fabs(tx) < 1e9 ? (int)rint(tx) : WINDOW_IDX_NONE;
            mys[u] = fabs(ty) < 1e9 ? (int)rint(ty) : WINDOW_IDX_NONE;
        }
    }
}

__global__ __launch_bounds__(256, UPDB_MIN_WAVES) void k_grid_update(Slam2dLidar lid, const Slam2dMap* __restrict__ maps, int P,
                                                           const double* __restrict__ pose, int pstride,
                                                           const double* __restrict__ ranges,
                                                           const int32_t* __restrict__ beam_shift, uint32_t* flags,
                                                           int groups, WeightsJob wj) {
    if (wj.abort_mask) {
        // scan-level abort (slam2d_scan_commit): if the match left one of these fault bits for ANY particle -- a search window
        // outside its map: the host has to grow the map and run the scan again -- nothing of this launch may happen: no map
        // update, no bookkeeping, no weights.  The bits were set by earlier launches and are not cleared here, so every
        // block reads the same.
        bool bad = false;
        const uint32_t* af = wj.abort_flags ? wj.abort_flags : flags;
        const int an = wj.abort_flags ? wj.abort_n : wj.N;
        // (with the device-side gate: a gate that gave up has left SLAM2D_F_SYNC_TIMEOUT in a group's fault word -- the scan is
        // voided like one whose window left a map, its report still reaches the host, which raises at once instead of waiting
        // for a sequence number that would never come)
        const uint32_t am = wj.abort_mask | (wj.nsync ? SLAM2D_F_SYNC_TIMEOUT : 0u);
        for (int i = threadIdx.x; i < an; i += blockDim.x) bad |= (af[i] & am) != 0u;
        if (__syncthreads_or(bad)) {
            if (blockIdx.x == 0 && wj.flag_snapshot)
                for (int i = threadIdx.x; i < wj.N; i += blockDim.x) wj.flag_snapshot[i] = flags[i] | SLAM2D_F_SCAN_VOIDED;
            // ... except that the report receives the COARSE matched poses: the host grows the maps for the fine windows round
            // them (Utils/ScanMatcher_OGBased.py:27 at the fine level) before it issues the scan again
            if (blockIdx.x == 0 && wj.report && wj.coarse)
                for (int i = threadIdx.x; i < wj.N; i += blockDim.x) {
                    wj.report[5 * i] = wj.coarse[i].x; wj.report[5 * i + 1] = wj.coarse[i].y; wj.report[5 * i + 2] = wj.coarse[i].theta;
                }
            if (blockIdx.x == 0) abort_arrive(wj);
            if (blockIdx.x == 0 && wj.nsync && wj.part && !wj.logw_all && threadIdx.x == 0) {
                // a sharded rank (the groups only arrive, the merge follows the all-gather on the normaliser's stream): the gate, the
                // collective and the merge of this scan are enqueued already, on every rank.  The group leaves the VOID partial
                // (sum < 0: no sum of exponentials is) and counts itself in -- not in its own word 2 + g: the scan comes again --
                // so the gate passes, every rank's merge finds the marker, merges nothing and reports the scan as voided
                // (slam2d_weights_merge_publish_report); the ranks that committed keep their partials and gather again.
                wj.part[0] = -INFINITY; wj.part[1] = -1.0; wj.part[2] = 0.0;
                __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
                __hip_atomic_fetch_add(&wj.nsync[0], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
            return;
        }
    }
    DBG_CLOCK(58, wj.logw && blockIdx.x == 0);
    if (wj.logw && blockIdx.x == 0) {                      // one extra block: the normaliser, beside the update (one launch less;
        //                                                    block 0, so that it starts with the launch and not as its tail)
        if (wj.nsync) normaliser_wait(wj.nsync, wj.gidx, flags);  // (device-merged groups: the previous scan's merge has reached the log-weights)
        if (wj.fine) {                                     // ... after the scan's bookkeeping (the update blocks take their
            for (int i = threadIdx.x; i < wj.N; i += blockDim.x) {        // poses from the match buffer themselves)
                post_match_one(wj.fine, wj.coarse, i, wj.prev, wj.heading, wj.logw, wj.report);
                if (wj.next_est)                                            // (reads what this very thread has just written)
                    prior_one(wj.prev, wj.heading, i, wj.next_raw_theta, wj.next_prev_raw_theta, wj.next_has_turn, wj.next_raw_turn,
                              wj.next_est, wj.next_psi);
            }
            for (int i = threadIdx.x; i < wj.pull_n; i += blockDim.x) wj.pull_dst[i] = __builtin_nontemporal_load(wj.pull_src + i);
            __syncthreads();
        }
        if (wj.part) {
            if (wj.flags && wj.flag_snapshot)              // (slam2d_groups_commit: the scan's fault bits move into the report)
                for (int i = threadIdx.x; i < wj.N; i += blockDim.x) wj.flag_snapshot[i] = atomicExch(&wj.flags[i], 0u);
            weights_local_body(wj.logw, wj.logconf, wj.cstride, wj.N, wj.part);
            if (wj.nsync) normaliser_arrive(wj);
        }
        else weights_body(wj.logw, wj.logconf, wj.cstride, wj.N, wj.w, wj.stats, wj.flags, wj.flag_snapshot, true);
        DBG_CLOCK(59, true);
        return;
    }
    const int bidx = blockIdx.x - (wj.logw ? 1 : 0);       // (a particle's blocks still share blockIdx.x % 8, i.e. their XCD)
    DBG_CLOCK(60, bidx == 0);
    const int xcd = bidx & 7, q = bidx >> 3;
    const int p = (q / groups) * 8 + xcd, g = q % groups;
    if (p >= P) return;
    const int W = lid.lut_w, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const Slam2dMap m = maps[p];
    const double px = pose[(size_t)p * pstride], py = pose[(size_t)p * pstride + 1], th = pose[(size_t)p * pstride + 2];
    const double inv_unit = 1.0 / lid.unit;
    uint32_t f = 0;
    // one wave per beam, UPDB_UNROLL chunks of 64 cells in flight: the walk is a chain of dependent loads
    // (list -> cell -> store), so the loads of several chunks are issued before the first use.  The map
    // index of a cell is computed per cell (window_map_index: tabulating both axes per block costs more than that)
    {
        const int beam = g * UPDB_BEAMS + wave;
        if (beam >= lid.beams) return;
        const double rg = ranges[beam];
        const double lo = rg - lid.wall_half, hi = rg + lid.wall_half;
        const bool returned = rg < lid.max_range;
        // a beam without return marks no free cells (:138) and starts at its wall band
        int kbeg, kwall, kend;
        if (!beam_bands(lid, beam_spoke(lid, th, beam), lo, hi, returned, kbeg, kwall, kend)) return;
        // the cells below the wall band are free by construction (most of a returned beam's cells): their radii are not read
        // (8 of a chunk's ~36 lines; UPDB_SKIP_R=0: read them all)
        const int klo = UPDB_SKIP_R ? kwall : kbeg;
        const double* __restrict__ sr = lid.spoke_r;
        const uint32_t* __restrict__ sc = lid.spoke_cells;
        // stale indices of a beam during which the map grew on a low side (:144-152): shift of the beam's own growth,
        // of the later beams' growths, and the map shape at the time of the write (Python wraps a negative index
        // against THAT shape) -- LidarModel.grow_for_update
        int sx = 0, sy = 0, ax = 0, ay = 0, wc = m.cols, wr = m.rows;
        if (beam_shift) {
            const int32_t* bs = beam_shift + ((size_t)p * lid.beams + beam) * 6;
            sx = bs[0]; sy = bs[1]; ax = bs[2]; ay = bs[3]; wc = bs[4]; wr = bs[5];
        }
        const uint32_t ncells = (uint32_t)m.rows * (uint32_t)m.pitch;
        const WindowLattice wl = window_lattice(lid, m, px, py, inv_unit);
        const bool lattice = !beam_shift && wl.on && !UPDB_NO_LATTICE;
        if (!lattice && !(lid.lut_xs_step > lid.unit * (1.0 + 1e-9))) {
            // One writer per map cell is the premise of the plain read-modify-write below.  Off the lattice it can fail: at a
            // pose on a half cell rint's ties-to-even sends two adjacent window columns (rows) to ONE map index (the window step
            // is never below the unit: only neighbours can meet), where the reference's fancy-index statement adds once per
            // statement (Utils/OccupancyGrid.py:149-152) and this kernel would add twice, or lose one of two increments that
            // share an instruction.  Decided once per wave from the W - 1 neighbour pairs of each axis, the same for every wave
            // of the particle: its map is then not touched at all and it gets SLAM2D_F_UPDATE_CELL_COLLISION -- the host raises
            // (slam2d_map_scans computes these poses exactly).  A window step above the unit by more than the quotients' rounding
            // error (< 1e-11 cells) keeps neighbours at least one index apart whatever the pose: those lidars skip the test.
            bool meet = false;
            for (int j = lane; j < W - 1; j += 64) {
                const double a0 = window_coord(lid, j), a1 = window_coord(lid, j + 1);
                meet |= rint(((px + a0) - m.lim_x0) / lid.unit) == rint(((px + a1) - m.lim_x0) / lid.unit) ||
                        rint(((py + a0) - m.lim_y0) / lid.unit) == rint(((py + a1) - m.lim_y0) / lid.unit);
            }
            if (__any(meet)) {
                if (lane == 0) atomicOr(&flags[p], SLAM2D_F_UPDATE_CELL_COLLISION);
                return;
            }
        }
        for (int k0 = kbeg + lane; k0 < kend; k0 += 64 * UPDB_UNROLL) {
            // straight-line phases, every load of a phase issued before its first use (no branches in between)
            double r[UPDB_UNROLL];
            uint32_t cell[UPDB_UNROLL], inc[UPDB_UNROLL], c[UPDB_UNROLL], at[UPDB_UNROLL];
            int mxs[UPDB_UNROLL], mys[UPDB_UNROLL];
            if ((k0 - lane) + 64 * UPDB_UNROLL <= klo) {        // (wave-uniform)
#pragma unroll
                for (int u = 0; u < UPDB_UNROLL; ++u) {
                    r[u] = -INFINITY;
                    cell[u] = sc[k0 + u * 64];
                }
            } else {
#pragma unroll
                for (int u = 0; u < UPDB_UNROLL; ++u) {
                    const int k = min(k0 + u * 64, kend - 1);
                    r[u] = sr[k];
                    cell[u] = sc[k];
                }
            }
            window_map_index<UPDB_UNROLL>(lid, m, px, py, inv_unit, lattice, wl.bx, wl.by, cell, mxs, mys);
#pragma unroll
            for (int u = 0; u < UPDB_UNROLL; ++u) {
                inc[u] = 0u;
                if (k0 + u * 64 < kend) {
                    if (returned && r[u] < lo) inc[u] = 1u;                      // :138-139,149
                    else if (r[u] > lo && r[u] < hi) inc[u] = 0x00020002u;       // :142-143,151-152
                }
                int mx = mxs[u] - sx, my = mys[u] - sy;
                if (beam_shift) {
                    mx -= ax; my -= ay;
                    if (mx < 0) mx += wc;
                    if (my < 0) my += wr;
                    mx += ax; my += ay;
                }
                if (inc[u] && (mx < 0 || mx >= m.cols || my < 0 || my >= m.rows)) { f |= SLAM2D_F_UPDATE_OUTSIDE_MAP; inc[u] = 0u; }
                mxs[u] = mx; mys[u] = my;
                at[u] = inc[u] ? (uint32_t)my * (uint32_t)m.pitch + (uint32_t)mx : 0u;     // cell 0: a harmless read
            }
            if (m.wide) {
                // 64-bit cells (visited << 32 | total): a map whose counts have outgrown 16 bits (the host promotes it before
                // that can happen; the reference's float64 counts never saturate, Utils/OccupancyGrid.py:148-152)
                unsigned long long* cells64 = reinterpret_cast<unsigned long long*>(m.cells);
                unsigned long long c64[UPDB_UNROLL];
#pragma unroll
                for (int u = 0; u < UPDB_UNROLL; ++u) c64[u] = cells64[min(at[u], ncells - 1u)];
#pragma unroll
                for (int u = 0; u < UPDB_UNROLL; ++u) {
                    if (!inc[u]) continue;
                    const unsigned long long add = inc[u] == 1u ? 1ull : 0x0000000200000002ull;
                    if (beam_shift) { atomicAdd(&cells64[at[u]], add); continue; }
                    const unsigned long long nc = c64[u] + add;
                    cells64[at[u]] = nc;
                    const bool was = 2ull * (c64[u] >> 32) > (c64[u] & 0xffffffffull), is = 2ull * (nc >> 32) > (nc & 0xffffffffull);
                    if (was != is) {
                        uint32_t* word = m.occ_bits + (size_t)mys[u] * m.bits_pitch + (mxs[u] >> 5);
                        if (is) atomicOr(word, 1u << (mxs[u] & 31)); else atomicAnd(word, ~(1u << (mxs[u] & 31)));
                    }
                }
                continue;
            }
#pragma unroll
            for (int u = 0; u < UPDB_UNROLL; ++u) c[u] = m.cells[min(at[u], ncells - 1u)];
#pragma unroll
            for (int u = 0; u < UPDB_UNROLL; ++u) {
                if (!inc[u]) continue;
                if ((c[u] & 0xffffu) + (inc[u] & 0xffffu) > 0xffffu) { f |= SLAM2D_F_COUNT_OVERFLOW; continue; }
                if (beam_shift) {
                    // stale-index writes can land on a cell of ANOTHER beam's spoke (the reference then adds both
                    // increments, Utils/OccupancyGrid.py:148-152): no plain read-modify-write here; the caller rebuilds
                    // the occupancy bits afterwards (slam2d_map_refresh_bits)
                    atomicAdd(&m.cells[at[u]], inc[u]);
                    continue;
                }
                const uint32_t nc = c[u] + inc[u];
                m.cells[at[u]] = nc;
                const bool was = 2u * (c[u] >> 16) > (c[u] & 0xffffu), is = 2u * (nc >> 16) > (nc & 0xffffu);
                if (was != is) {                                       // keep the occupancy bit in step
                    uint32_t* word = m.occ_bits + (size_t)mys[u] * m.bits_pitch + (mxs[u] >> 5);
                    if (is) atomicOr(word, 1u << (mxs[u] & 31)); else atomicAnd(word, ~(1u << (mxs[u] & 31)));
                }
            }
        }
    }
    DBG_CLOCK(62, bidx == 0);
    if (f) atomicOr(&flags[p], f);
}

// ---- mapping from known poses (Utils/OccupancyGrid.py:main: updateOccupancyGrid per scan at given poses) ----
// Both kernels take S scans x B beams, one wave per (scan, beam), MAPS_BEAMS adjacent beams of one scan per block, and walk
// the beam's spoke cells by radial band as k_grid_update does.
#define MAPS_BEAMS 4

// Exact fp64 extent of the occupied points x + xAtSpokeDir[occ], y + yAtSpokeDir[occ] of every (scan, beam) (:142-147):
// out[(s * B + b) * 4 + 0..3] = (min x, max x, min y, max y), +inf / -inf for a beam without occupied cells.  checkMapToExpand
// (:108-118) only asks any(x < lim) and its kin, so these four numbers replay a beam's growth exactly.
__global__ __launch_bounds__(64 * MAPS_BEAMS) void k_occ_extent(Slam2dLidar lid, int S, int groups, const double* __restrict__ pose,
                                                               int pstride, const double* __restrict__ ranges, double* __restrict__ out) {
    const int s = blockIdx.x / groups, beam = (blockIdx.x % groups) * MAPS_BEAMS + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (s >= S || beam >= lid.beams) return;
    const double px = pose[(size_t)s * pstride], py = pose[(size_t)s * pstride + 1], th = pose[(size_t)s * pstride + 2];
    const double rg = ranges[(size_t)s * lid.beams + beam];
    const double lo = rg - lid.wall_half, hi = rg + lid.wall_half;
    double x0 = INFINITY, x1 = -INFINITY, y0 = INFINITY, y1 = -INFINITY;
    int kbeg, kwall, kend;
    if (beam_bands(lid, beam_spoke(lid, th, beam), lo, hi, false, kbeg, kwall, kend)) {
        for (int k = kbeg + lane; k < kend; k += 64) {
            const double r = lid.spoke_r[k];
            if (!(r > lo && r < hi)) continue;                                     // :142-143
            const uint32_t c = lid.spoke_cells[k];
            const double x = px + lid.lut_xs[c & 0xffffu], y = py + lid.lut_xs[c >> 16];
            x0 = fmin(x0, x); x1 = fmax(x1, x); y0 = fmin(y0, y); y1 = fmax(y1, y);
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        x0 = fmin(x0, __shfl_xor(x0, o)); x1 = fmax(x1, __shfl_xor(x1, o));
        y0 = fmin(y0, __shfl_xor(y0, o)); y1 = fmax(y1, __shfl_xor(y1, o));
    }
    if (lane == 0) {
        double* o = out + ((size_t)s * lid.beams + beam) * 4;
        o[0] = x0; o[1] = x1; o[2] = y0; o[3] = y1;
    }
}

// convertRealXYToMapIdx of one window coordinate (:104-105) against the limit in force when the beam's indices are taken;
// INT_MIN: not representable (a cell that far off is outside the map in any case)
__device__ __forceinline__ int stale_idx(double p, double xs, double lim0, double unit) {
    const double t = ((p + xs) - lim0) / unit;
    return fabs(t) < 1e9 ? (int)rint(t) : INT_MIN;
}

// The window columns j' of one row-or-column axis whose stale index is v: the neighbours of j for v == a (its own index), and
// the columns about (v - a) * unit / step further on for the wrapped alias v == a + n.  The index is non-decreasing in j and
// the window step is in [unit, 2 unit), so no value is taken by more than two columns.  Writes (column, wrapped) pairs.
__device__ __forceinline__ int axis_partners(const Slam2dLidar& lid, double p, double lim0, int j, int a, int n, int* col, int* wrapped) {
    const int W = lid.lut_w;
    int k = 0;
    col[k] = j; wrapped[k++] = a < 0;
    if (j > 0 && stale_idx(p, lid.lut_xs[j - 1], lim0, lid.unit) == a) { col[k] = j - 1; wrapped[k++] = a < 0; }
    if (j + 1 < W && stale_idx(p, lid.lut_xs[j + 1], lim0, lid.unit) == a) { col[k] = j + 1; wrapped[k++] = a < 0; }
    if (a < 0) {
        // Python's wrap: a negative index a names element a + n; a cell of the same statement whose index IS a + n writes there too
        const double step = (lid.lut_xs[W - 1] - lid.lut_xs[0]) / (double)(W - 1);
        const int jc = j + (int)floor((double)n * lid.unit / step);
        for (int t = jc - 1; t <= jc + 2; ++t)
            if (t >= 0 && t < W && k < 6 && stale_idx(p, lid.lut_xs[t], lim0, lid.unit) == a + n) { col[k] = t; wrapped[k++] = 0; }
    }
    return k;
}

// updateOccupancyGrid (:127-152) for S scans at given poses into ONE map, the reference's semantics exactly:
//  - indices are taken against the limits in force for that beam (plan[s][b].lim_*: after the earlier beams' and scans' growth,
//    before the beam's own), wrap Python-style against the shape right after the beam's growth (cols, rows) and move with every
//    later low-side growth of the batch (ac, ar) -- the map is already grown to the batch's final extent;
//  - one fancy-index statement (a beam's empty cells; its occupied cells) adds to each element it names ONCE, however many of its
//    cells name it: two adjacent window columns (rows) share an index when a pose sits on a half cell, or -- after a wrap --
//    an index a < 0 and a + cols name one element.  Of the cells of a statement that name one element, the one first in the order
//    (number of wrapped axes, window row, window column) writes; the others find it among their partners and stay silent;
//  - statements add up: integer atomics, so the counts do not depend on the order in which the waves run.
// The occupancy bits are NOT maintained (slam2d_map_refresh_bits afterwards).
__global__ __launch_bounds__(64 * MAPS_BEAMS) void k_map_scans(Slam2dLidar lid, const Slam2dMap* __restrict__ map, int S, int groups,
                                                              const double* __restrict__ pose, int pstride,
                                                              const double* __restrict__ ranges, const Slam2dBeamPlan* __restrict__ plan,
                                                              const uint16_t* __restrict__ lut_bin, const double* __restrict__ lut_r,
                                                              uint32_t* flags) {
    const int s = blockIdx.x / groups, beam = (blockIdx.x % groups) * MAPS_BEAMS + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (s >= S || beam >= lid.beams) return;
    const Slam2dMap m = *map;
    const Slam2dBeamPlan pl = plan[(size_t)s * lid.beams + beam];
    const double px = pose[(size_t)s * pstride], py = pose[(size_t)s * pstride + 1], th = pose[(size_t)s * pstride + 2];
    const double rg = ranges[(size_t)s * lid.beams + beam];
    const double lo = rg - lid.wall_half, hi = rg + lid.wall_half;
    const bool returned = rg < lid.max_range;
    const int W = lid.lut_w, spoke = beam_spoke(lid, th, beam);
    int kbeg, kwall, kend;
    if (!beam_bands(lid, spoke, lo, hi, returned, kbeg, kwall, kend)) return;
    uint32_t f = 0;
    for (int k = kbeg + lane; k < kend; k += 64) {
        const double r = lid.spoke_r[k];
        const int cls = (returned && r < lo) ? 1 : (r > lo && r < hi) ? 2 : 0;       // :138-143
        if (!cls) continue;
        const uint32_t c = lid.spoke_cells[k];
        const int j = (int)(c & 0xffffu), i = (int)(c >> 16);
        const int ax = stale_idx(px, lid.lut_xs[j], pl.lim_x0, lid.unit), ay = stale_idx(py, lid.lut_xs[i], pl.lim_y0, lid.unit);
        const int ex = ax < 0 && ax != INT_MIN ? ax + pl.cols : ax, ey = ay < 0 && ay != INT_MIN ? ay + pl.rows : ay;
        if (ex < 0 || ex >= pl.cols || ey < 0 || ey >= pl.rows ||              // (the reference: IndexError)
            ex + pl.ac >= m.cols || ey + pl.ar >= m.rows) { f |= SLAM2D_F_UPDATE_OUTSIDE_MAP; continue; }
        int cj[6], wj[6], ci[6], wi[6];
        const int ncj = axis_partners(lid, px, pl.lim_x0, j, ax, pl.cols, cj, wj);
        const int nci = axis_partners(lid, py, pl.lim_y0, i, ay, pl.rows, ci, wi);
        bool silent = false;
        if (ncj > 1 || nci > 1) {
            const int mine = wj[0] + wi[0];
            for (int u = 0; u < nci && !silent; ++u)
                for (int v = 0; v < ncj && !silent; ++v) {
                    const int ii = ci[u], jj = cj[v], theirs = wi[u] + wj[v];
                    if (!(theirs < mine || (theirs == mine && (ii < i || (ii == i && jj < j))))) continue;
                    const size_t q = (size_t)ii * W + jj;
                    if (lut_bin[q] != spoke) continue;
                    const double rq = lut_r[q];
                    silent = cls == 1 ? rq < lo : (rq > lo && rq < hi);
                }
        }
        if (silent) continue;
        const size_t at = (size_t)(ey + pl.ar) * m.pitch + (size_t)(ex + pl.ac);
        if (m.wide) {
            atomicAdd(reinterpret_cast<unsigned long long*>(m.cells) + at, cls == 1 ? 1ull : 0x0000000200000002ull);
        } else {
            const uint32_t inc = cls == 1 ? 1u : 0x00020002u;
            const uint32_t old = atomicAdd(m.cells + at, inc);
            if ((old & 0xffffu) + (inc & 0xffffu) > 0xffffu) f |= SLAM2D_F_COUNT_OVERFLOW;   // (the host promotes before this can happen)
        }
    }
    if (f) atomicOr(flags, f);
}

// ---- the scan a map expects at a pose (slam2d_predict_scan): the inverse of the update, in the update's discretisation ----
// The update writes a beam's wall into the cells of ONE spoke of the window (Utils/OccupancyGrid.py:131-152); the range a map
// predicts for the beam is therefore the nearest occupied cell of that spoke: a min, a max and a count over table radii.
#define PRED_UNROLL 4
#define PRED_KEEP 1                  // chunks of 64 * PRED_UNROLL cells whose hits k_predict_scan keeps in registers for the wall

// The cells k = kb + lane + 64 u (u < PRED_UNROLL) of one spoke list: rr[u] = the cell's tabulated radius where it is a HIT -- k < kend,
// its map index inside the map, its occupancy bit set, r_min < r < r_max -- and +inf elsewhere.  Straight-line phases, every load
// of a phase issued before its first use: the walk is a chain list -> cell -> bit word.  The map index is the update's own
// (window_map_index, the lattice decided once per wave by the caller).  A cell outside the map reads bit word 0 and discards
// it: no access leaves the map.
__device__ __forceinline__ void predict_hits(const Slam2dLidar& lid, const Slam2dMap& m, const int kb, const int kend, const int lane,
                                             const double px, const double py, const double inv_unit, const bool lattice,
                                             const int bx, const int by, const double r_min, const double r_max,
                                             double (&rr)[PRED_UNROLL]) {
    double r[PRED_UNROLL];
    uint32_t cell[PRED_UNROLL], word[PRED_UNROLL];
    int mxs[PRED_UNROLL], mys[PRED_UNROLL];
#pragma unroll
    for (int u = 0; u < PRED_UNROLL; ++u) {
        const int k = min(kb + lane + u * 64, kend - 1);
        r[u] = lid.spoke_r[k];
        cell[u] = lid.spoke_cells[k];
    }
    window_map_index<PRED_UNROLL>(lid, m, px, py, inv_unit, lattice, bx, by, cell, mxs, mys);
    bool inside[PRED_UNROLL];
#pragma unroll
    for (int u = 0; u < PRED_UNROLL; ++u) {
        inside[u] = mxs[u] >= 0 && mxs[u] < m.cols && mys[u] >= 0 && mys[u] < m.rows;
        word[u] = m.occ_bits[inside[u] ? (size_t)mys[u] * (size_t)m.bits_pitch + (size_t)(mxs[u] >> 5) : (size_t)0];
    }
#pragma unroll
    for (int u = 0; u < PRED_UNROLL; ++u) {
        const bool hit = inside[u] && ((word[u] >> (mxs[u] & 31)) & 1u) && kb + lane + u * 64 < kend && r[u] > r_min && r[u] < r_max;
        rr[u] = hit ? r[u] : INFINITY;
    }
}

// One wave per (pose, beam), MAPS_BEAMS adjacent beams of one pose per block.  out[(s * beams + b) * SLAM2D_PREDICT_STRIDE + 0..3] =
// (r_hit, r_far, n_hit, 0): the smallest radius over the beam's hits, and the largest radius and the number of the hits with
// r < r_hit + wallThickness -- the wall the update would have put there; (+inf, -inf, 0, 0) for a beam without a hit.
// The cells of a spoke are ordered by radial band and floor(r / unit) is monotone in r, so r_hit lies in the first band that holds
// a hit, and the wall's cells in the bands up to the one that holds r_hit + wallThickness: the walk stops behind that band (a
// wave-uniform exit).  Work follows the cells up to the first wall, as the update's, not the window.
__global__ __launch_bounds__(64 * MAPS_BEAMS) void k_predict_scan(Slam2dLidar lid, const Slam2dMap* __restrict__ maps, int map_stride, int S,
                                                                 int groups, const double* __restrict__ pose, int pstride,
                                                                 double r_min, double r_max, double* __restrict__ out) {
    const int s = blockIdx.x / groups, beam = (blockIdx.x % groups) * MAPS_BEAMS + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (s >= S || beam >= lid.beams) return;
    const Slam2dMap m = maps[(size_t)s * map_stride];
    const double px = pose[(size_t)s * pstride], py = pose[(size_t)s * pstride + 1], th = pose[(size_t)s * pstride + 2];
    double r_hit = INFINITY, r_far = -INFINITY;
    int n_hit = 0;
    // A pose with a non-finite component, or one whose heading quotient or window-edge quotients are not below 1e9, sees nothing:
    // decided here, before any conversion to an integer (the quotients of the cells in between lie between those of the edges)
    const double R = lid.max_range;
    const bool valid = isfinite(px) && isfinite(py) && isfinite(th) && fabs(th / (2 * 3.141592653589793) * (double)lid.num_spokes) < 1e9 &&
                       fabs(((px + -R) - m.lim_x0) / lid.unit) < 1e9 && fabs(((px + R) - m.lim_x0) / lid.unit) < 1e9 &&
                       fabs(((py + -R) - m.lim_y0) / lid.unit) < 1e9 && fabs(((py + R) - m.lim_y0) / lid.unit) < 1e9;
    if (valid && m.rows > 0 && m.cols > 0 && m.occ_bits) {
        const int nb = lid.num_bands, spoke = beam_spoke(lid, th, beam);
        const int* __restrict__ bp = spoke_bands(lid, spoke);
        int kbeg = 0, kwall = 0, kend = 0;                                     // (an empty walk; never left so: the host admits
        beam_bands(lid, spoke, r_min, r_max, false, kbeg, kwall, kend);        //  0 <= r_min < r_max only)
        const double inv_unit = 1.0 / lid.unit;
        const WindowLattice wl = window_lattice(lid, m, px, py, inv_unit);
        // the band starts of the spoke, one per lane (a table of more than 64 entries is read from memory): the walk's limits
        // follow the nearest hit found so far, and a load from the table there would sit in the chain of every chunk
        const int bp_lane = (nb < 64 && lane <= nb) ? bp[lane] : 0;
        auto band_start = [&](const int i) { return nb < 64 ? __shfl(bp_lane, i) : bp[i]; };
        const double wall = lid.wall_half + lid.wall_half;
        // ONE walk where it can be: the hits of up to PRED_KEEP chunks that hold any stay in registers
        // while the walk goes on to the end of the band that holds r_hit + wallThickness (the limit only moves inwards as r_hit
        // falls, and never before the end of r_hit's own band, so r_hit is final when the walk ends); the wall is then taken
        // from the kept chunks.  A wall spread over more chunks than that is walked again from the band of r_hit.
        double keep[PRED_KEEP][PRED_UNROLL];
        int fb = 0, klim = kend, nkept = 0;
        for (int kb = kbeg; kb < klim; kb += 64 * PRED_UNROLL) {
            double rr[PRED_UNROLL];
            predict_hits(lid, m, kb, kend, lane, px, py, inv_unit, wl.on, wl.bx, wl.by, r_min, r_max, rr);
            double lr = rr[0];
#pragma unroll
            for (int u = 1; u < PRED_UNROLL; ++u) lr = fmin(lr, rr[u]);
            const bool any = __ballot(lr < INFINITY) != 0ull;        // (wave-uniform)
            if (any) {                                                // (a chunk without a hit has nothing for the wall)
#pragma unroll
                for (int q = 0; q < PRED_KEEP; ++q)
                    if (nkept == q) {
#pragma unroll
                        for (int u = 0; u < PRED_UNROLL; ++u) keep[q][u] = rr[u];
                    }
                ++nkept;
                r_hit = fmin(r_hit, wave64_min(lr));
                fb = min((int)fmin(floor(r_hit / lid.unit), 2.0e9) / SLAM2D_SPOKE_BAND, nb - 1);
                const int qw = (int)fmin(floor((r_hit + wall) / lid.unit), 2.0e9);
                klim = min(kend, band_start(min(qw / SLAM2D_SPOKE_BAND + 1, nb)));
            }
        }
        if (r_hit < INFINITY) {
            const double wall_end = r_hit + wall;
            double far = -INFINITY;
            if (nkept <= PRED_KEEP) {
#pragma unroll
                for (int q = 0; q < PRED_KEEP; ++q)
                    if (q < nkept) {
#pragma unroll
                        for (int u = 0; u < PRED_UNROLL; ++u) {
                            const bool in_wall = keep[q][u] < wall_end;
                            if (in_wall) far = fmax(far, keep[q][u]);
                            n_hit += __popcll(__ballot(in_wall));
                        }
                    }
            } else {
                const int wbeg = max(kbeg, band_start(fb));
                for (int kb = wbeg; kb < klim; kb += 64 * PRED_UNROLL) {
                    double rr[PRED_UNROLL];
                    predict_hits(lid, m, kb, klim, lane, px, py, inv_unit, wl.on, wl.bx, wl.by, r_min, r_max, rr);
#pragma unroll
                    for (int u = 0; u < PRED_UNROLL; ++u) {
                        const bool in_wall = rr[u] < wall_end;
                        if (in_wall) far = fmax(far, rr[u]);
                        n_hit += __popcll(__ballot(in_wall));
                    }
                }
            }
            r_far = wave64_max(far);
        }
    }
    if (lane == 0) {
        double* o = out + ((size_t)s * lid.beams + beam) * SLAM2D_PREDICT_STRIDE;
        o[0] = r_hit; o[1] = r_far; o[2] = (double)n_hit; o[3] = 0.0;
    }
}

// ---- a scan's score at any poses in a level's field (slam2d_score_poses): the front half of k_endpoints without its angle loop ----
// What the sweep sums for one pose of a cube (Utils/ScanMatcher_OGBased.py:81-89,117-121,129-130,173-176), for N free poses: the
// cost of the SET of field cells the in-range beams end in (np.unique, :120), an integer sum, so whichever beam claims a cell the
// result is the same bits.
#define SCORE_WAVES 4                // poses (waves) per block while four hash sets stay within 32 KB; two beyond (score_hash_size() == 4096)

// slots of a pose's hash set of cell keys: a power of two >= 1.5 * beams (load factor <= 2/3: an empty slot ends every probe), >= 64
__host__ __device__ __forceinline__ int score_hash_size(const int beams) {
    int h = 64;
    while (h < beams + ((beams + 1) >> 1)) h <<= 1;
    return h;
}
__device__ __forceinline__ unsigned long long wave64_sum_u64(const unsigned long long v) {      // (all 64 lanes active)
    const unsigned long long t = row16_sum_u64(v);
    unsigned long long s = 0ull;
#pragma unroll
    for (int l = 0; l < 64; l += 16)
        s += ((unsigned long long)(unsigned)__builtin_amdgcn_readlane((int)(unsigned)(t >> 32), l) << 32) |
             (unsigned)__builtin_amdgcn_readlane((int)(unsigned)t, l);
    return s;
}

// The beam-to-cell step of slam2d_score_poses and slam2d_search_lattice (include/slam2d.h, steps 3-4 of the former): the field
// cell an endpoint falls in, and whether the beam is INSIDE.  The true division; a quotient that fails the guard -- a NaN fails
// it -- never reaches the conversion; truncation as astype(int) has it.
__device__ __forceinline__ bool score_cell(const double px, const double py, const double xlo, const double ylo, const double step,
                                           const int fw, const int fh, int& cx, int& cy) {
    const double qx = (px - xlo) / step, qy = (py - ylo) / step;                 // :174-175
    if (!(fabs(qx) < 1e9 && fabs(qy) < 1e9)) return false;
    cx = (int)qx;
    cy = (int)qy;
    return cx >= 0 && cx < fw && cy >= 0 && cy < fh;
}

// What every kernel of this layer reads of a level's slot p_field: its frame, the frame's clipped size, its field image
struct SlotField { Slam2dFrame fr; FieldSize fs; const uint32_t* field; };
__device__ __forceinline__ SlotField slot_field(const Slam2dLevel& lv, const int p_field) {
    const Slam2dFrame fr = lv.frames[p_field];
    return SlotField{fr, frame_clip(lv, fr), lv.field + (size_t)p_field * lv.fmax * lv.fpitch};
}

// One wave per pose, blockDim.x / 64 poses per block, beams interleaved over the lanes (beam = 64 i + lane: a wave's range loads
// are contiguous).  out[n * SLAM2D_SCORE_STRIDE + 0..7] as include/slam2d.h lists them.  The hash set holds keys only: the lane
// whose atomicCAS finds a slot empty owns the cell and adds its cost to sum_u, every inside beam adds to sum_b.  The wave's
// hash set is its own, so the one barrier only orders its clearing before the insertions.  Reads frames[p_field], the slot's
// field and the inputs; writes out; no global atomic, no fault bit.
__global__ __launch_bounds__(64 * SCORE_WAVES) void k_score_poses(Slam2dLidar lid, Slam2dLevel lv, int p_field, int N, int hsize,
                                                                  const double* __restrict__ pose, int pstride,
                                                                  const double* __restrict__ ranges, int rstride,
                                                                  double* __restrict__ out) {
    extern __shared__ __attribute__((aligned(16))) int score_lds[];              // [blockDim.x / 64][hsize] keys
    const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int n = blockIdx.x * (blockDim.x >> 6) + wv;
    int* hkey = score_lds + wv * hsize;
    const int hmask = hsize - 1;
    for (int i = lane; i < hsize; i += 64) hkey[i] = INT_MAX;                    // (no key: cx < 2^15 leaves the low half below 0xffff)
    __syncthreads();
    if (n >= N) return;                                                          // (wave-uniform)
    const SlotField sf = slot_field(lv, p_field);
    const double x = pose[(size_t)n * pstride], y = pose[(size_t)n * pstride + 1], th = pose[(size_t)n * pstride + 2];
    const double* __restrict__ rg = ranges + (size_t)n * rstride;
    const int B = lid.beams;
    const BeamFan fan = fan_of(lid, th);
    unsigned long long sum_u = 0ull, sum_b = 0ull;                               // (this lane's share)
    int n_u = 0, n_in = 0, n_rng = 0;                                            // (the wave's counts: ballots)
    for (int b0 = 0; b0 < B; b0 += 64) {                                         // (wave-uniform trip count)
        const int b = b0 + lane;
        const double r = b < B ? rg[b] : NAN;
        const bool in_range = r < lid.max_range;                                 // :84 (NaN and +inf are out, 0 and negatives in)
        bool inside = false;
        int key = INT_MAX;
        uint32_t cost = 0u;
        if (in_range) {
            const double a = fan.angle(b);
            const double px = x + cos(a) * r, py = y + sin(a) * r;               // :87-88
            int cx, cy;
            if (score_cell(px, py, sf.fr.xlo, sf.fr.ylo, lv.step, sf.fs.fw, sf.fs.fh, cx, cy)) {
                inside = true;
                key = (cy << 16) | cx;
                cost = sf.field[(size_t)cy * lv.fpitch + cx];
            }
        }
        bool owns = false;
        if (inside) {
            int slot;
            owns = cell_set_insert(hkey, hmask, key, slot);
            sum_b += cost;
            if (owns) sum_u += cost;
        }
        n_rng += __popcll(__ballot(in_range));
        n_in += __popcll(__ballot(inside));
        n_u += __popcll(__ballot(owns));
    }
    sum_u = wave64_sum_u64(sum_u);
    sum_b = wave64_sum_u64(sum_b);
    if (lane == 0) {
        const double inv = 1.0 / lv.cost_scale;
        double* o = out + (size_t)n * SLAM2D_SCORE_STRIDE;
        o[0] = -((double)sum_u * inv); o[1] = (double)n_u; o[2] = -((double)sum_b * inv); o[3] = (double)n_in;
        o[4] = (double)n_rng; o[5] = (double)sum_u; o[6] = (double)sum_b; o[7] = 0.0;
    }
}

// ---- a geometric ray in a field's frame (slam2d_cast_rays, slam2d_score_rays): include/slam2d.h states the ray, DESIGN.md
// section 4 proves the skip rule ----
#define RAY_WAVES 4                  // waves per block of both kernels: a wave is 64 beams of a pose (cast) or a pose (score)

// What a ray reads of its slot: the frame's origin and clipped size, the step, the slot's squared-distance image
struct RayField { double xlo, ylo, step; int fw, fh, pitch; const uint32_t* __restrict__ d2; };
__device__ __forceinline__ RayField ray_field(const Slam2dLevel& lv, const int p_field, const uint32_t* __restrict__ dist2) {
    const Slam2dFrame fr = lv.frames[p_field];
    const FieldSize fs = frame_clip(lv, fr);
    return RayField{fr.xlo, fr.ylo, lv.step, fs.fw, fs.fh, lv.fpitch, dist2 + (size_t)p_field * lv.fmax * lv.fpitch};
}

// Sample k of the ray from (x, y) along (c, s): INSIDE or not, and its cell.  One rounded operation at a time, in the header's
// order; a quotient that fails the guard -- a NaN, a negative one: the `0 <=` is the ray's, not the endpoint's -- never reaches
// the conversion.
__device__ __forceinline__ bool ray_sample(const RayField& f, const double x, const double y, const double c, const double s, const int k,
                                           int& cx, int& cy) {
    const double t = (double)k * f.step;
    const double px = x + c * t, py = y + s * t;
    const double qx = (px - f.xlo) / f.step, qy = (py - f.ylo) / f.step;
    if (!(qx >= 0.0 && qx < 1e9 && qy >= 0.0 && qy < 1e9)) return false;
    cx = (int)qx;
    cy = (int)qy;
    return cx < f.fw && cy < f.fh;
}

// floor(sqrt(v)) of a 32-bit value: the float root is within one of it, and one step either way settles it
__device__ __forceinline__ uint32_t ray_isqrt(const uint32_t v) {
    uint32_t d = (uint32_t)__fsqrt_rn((float)v);
    d = min(d, 65535u);
    if (d * d > v) --d;
    else if (d < 65535u && (d + 1u) * (d + 1u) <= v) ++d;
    return d;
}

// The ray of one lane up to sample `limit` (0 <= limit < 2^30): kind << 30 | k as slam2d_cast_rays writes it.  Every lane of the
// wave calls it; a lane with !active walks nothing and gets RAY_NONE.
//   Frame exit: every operation of the sample formula is monotone in k, so the inside samples of a ray are one interval of k;
// with sample 0 inside, its end k_exit is found by bisection -- arithmetic only -- and the walk runs on [0, min(limit + 1,
// k_exit)) without ever looking for the first outside sample.
//   Skip rule: at an examined sample in a cell of value v > 0, D = isqrt(v), no sample before k + max(1, D - 1) can lie in an
// occupied cell (samples are one cell apart, a sample within 0.7072 of its cell's centre), so that is the next one examined.
//   The loop is wave-uniform: it ends when no lane is live, finished lanes idle.  A ray is a chain of dependent 4-byte gathers.
__device__ __forceinline__ uint32_t ray_walk(const RayField& f, const double x, const double y, const double c, const double s, const int limit,
                                             const bool active) {
    int cx = 0, cy = 0;
    uint32_t word = (SLAM2D_RAY_NONE << 30) | (uint32_t)(limit + 1);
    bool live = active;
    int k_exit = limit + 1;
    if (live && !ray_sample(f, x, y, c, s, 0, cx, cy)) {                            // (a non-finite pose ends here too)
        word = SLAM2D_RAY_LEFT << 30;
        live = false;
    }
    if (live) {
        int lo = 0;                                                              // (inside), k_exit: outside, or limit + 1
        while (k_exit - lo > 1) {
            const int mid = lo + ((k_exit - lo) >> 1);
            int ux, uy;
            if (ray_sample(f, x, y, c, s, mid, ux, uy)) lo = mid; else k_exit = mid;
        }
        if (k_exit <= limit) word = (SLAM2D_RAY_LEFT << 30) | (uint32_t)k_exit;
    }
    int k = 0;
    while (__ballot(live)) {
        if (live) {
            const uint32_t v = f.d2[(size_t)cy * f.pitch + cx];                  // (cx, cy): sample k, inside
            if (v == 0u) {
                word = (SLAM2D_RAY_HIT << 30) | (uint32_t)k;
                live = false;
            } else {
                const uint32_t d = ray_isqrt(v);
                k += d > 2u ? (int)d - 1 : 1;
                live = k < k_exit && ray_sample(f, x, y, c, s, k, cx, cy);        // (k < k_exit is inside: the guard runs all the same)
            }
        }
    }
    return word;
}

// slam2d_cast_rays: wave w of the launch is beams 64 g .. 64 g + 63 of pose n, w = n * groups + g; a lane per beam.
__global__ __launch_bounds__(64 * RAY_WAVES) void k_cast_rays(Slam2dLidar lid, Slam2dLevel lv, int p_field, const uint32_t* __restrict__ dist2,
                                                              int N, int groups, const double* __restrict__ pose, int pstride, int K,
                                                              uint32_t* __restrict__ out) {
    const int lane = threadIdx.x & 63;
    const long long w = (long long)blockIdx.x * RAY_WAVES + (threadIdx.x >> 6);
    if (w >= (long long)N * groups) return;                                      // (wave-uniform)
    const int n = (int)(w / groups), b = (int)(w % groups) * 64 + lane;
    const RayField f = ray_field(lv, p_field, dist2);
    const double x = pose[(size_t)n * pstride], y = pose[(size_t)n * pstride + 1], th = pose[(size_t)n * pstride + 2];
    const bool active = b < lid.beams;
    const double a = fan_of(lid, th).angle(active ? b : 0);
    const uint32_t word = ray_walk(f, x, y, cos(a), sin(a), K, active);
    if (active) out[(size_t)n * lid.beams + b] = word;
}

// slam2d_score_rays: k_score_poses' shape -- a wave per pose, beams interleaved over the lanes -- without its hash set: the
// endpoint lookup of steps 1-4, then the ray of every CHECKED beam with kend >= 0 up to kend.  A pose is one wave, so its
// integer sums are joined by the DPP wave reduction alone; lane 0 writes the row.
__global__ __launch_bounds__(64 * RAY_WAVES) void k_score_rays(Slam2dLidar lid, Slam2dLevel lv, int p_field, const uint32_t* __restrict__ dist2,
                                                               int N, const double* __restrict__ pose, int pstride,
                                                               const double* __restrict__ ranges, int rstride, int margin,
                                                               uint32_t outside_cost, uint32_t through_cost, double* __restrict__ out) {
    const int lane = threadIdx.x & 63;
    const int n = blockIdx.x * RAY_WAVES + (threadIdx.x >> 6);
    if (n >= N) return;                                                          // (wave-uniform)
    const RayField f = ray_field(lv, p_field, dist2);
    const uint32_t* __restrict__ field = lv.field + (size_t)p_field * lv.fmax * lv.fpitch;
    const double x = pose[(size_t)n * pstride], y = pose[(size_t)n * pstride + 1], th = pose[(size_t)n * pstride + 2];
    const double* __restrict__ rg = ranges + (size_t)n * rstride;
    const int B = lid.beams;
    const BeamFan fan = fan_of(lid, th);
    unsigned long long sum_b = 0ull, sum_depth = 0ull;                           // (this lane's share)
    int n_in = 0, n_rng = 0, n_thr = 0, n_chk = 0;                               // (the wave's counts: ballots)
    for (int b0 = 0; b0 < B; b0 += 64) {                                         // (wave-uniform trip count)
        const int b = b0 + lane;
        const double r = b < B ? rg[b] : NAN;
        const bool in_range = r < lid.max_range;                                 // (NaN and +inf are out, 0 and negatives in)
        const double a = fan.angle(b < B ? b : 0);
        const double c = cos(a), s = sin(a);
        bool inside = false;
        if (in_range) {
            int cx, cy;
            if (score_cell(x + c * r, y + s * r, f.xlo, f.ylo, f.step, f.fw, f.fh, cx, cy)) {
                inside = true;
                sum_b += field[(size_t)cy * f.pitch + cx];
            }
        }
        const double q = r / f.step;
        const bool checked = in_range && q >= 0.0 && q < 1e9;
        const long long kend = checked ? (long long)q - margin : -1ll;
        const uint32_t word = ray_walk(f, x, y, c, s, kend >= 0 ? (int)kend : 0, kend >= 0);
        const bool through = kend >= 0 && (word >> 30) == SLAM2D_RAY_HIT;           // (a HIT lies at k <= the limit, kend)
        if (through) sum_depth += (unsigned long long)(kend - (long long)(word & 0x3fffffffu));
        n_rng += __popcll(__ballot(in_range));
        n_in += __popcll(__ballot(inside));
        n_chk += __popcll(__ballot(checked));
        n_thr += __popcll(__ballot(through));
    }
    sum_b = wave64_sum_u64(sum_b);
    sum_depth = wave64_sum_u64(sum_depth);
    if (lane == 0) {
        const unsigned long long cost = sum_b + (unsigned long long)(n_rng - n_in) * outside_cost + (unsigned long long)n_thr * through_cost;
        double* o = out + (size_t)n * SLAM2D_RAYS_STRIDE;
        o[0] = (double)cost; o[1] = (double)sum_b; o[2] = (double)n_in; o[3] = (double)n_rng;
        o[4] = (double)n_thr; o[5] = (double)n_chk; o[6] = (double)sum_depth; o[7] = 0.0;
    }
}

// ---- the best heading and its cost at every position of a lattice of poses (slam2d_search_lattice) ----
#define SEARCH_CHUNK 8              // headings one block row takes at least (tests/test_gpu_search.py names it)
#define SEARCH_UNROLL 4              // beams of one trip of the search's inner loop: their table entries and gathers are in flight together
#define SEARCH_WAVES 4096            // waves that fill the card: 256 CUs x 4 SIMDs x 4; windows with fewer split their headings further

// headings per block row (gridDim.y rows): at least SEARCH_CHUNK, more where the positions alone fill the card
__host__ __device__ __forceinline__ int search_chunk(const long long positions, const int nth) {
    const long long waves = (positions + WAVE - 1) / WAVE;
    const long long rows = (SEARCH_WAVES + waves - 1) / waves;                   // (>= 1)
    const long long hc = ((long long)nth + rows - 1) / rows;
    return hc > SEARCH_CHUNK ? (int)hc : SEARCH_CHUNK;
}

// First launch: E[it][k] = (cos(a_b) * r_b, sin(a_b) * r_b) of heading it and the k-th beam IN RANGE, b -- the only cos / sin of the
// search, the products rounded here so that x + e is x + cos(a) * r bit for bit (no
// contraction).  Which beams are in range does not depend on the pose: every heading's row is compacted alike, k = the number of
// beams in range below b (the lanes of a wave read ranges[j] at one address), and the search sums integers, in any order.  Also
// d_out = all ones, the identity of the search launch's atomicMin.
__global__ __launch_bounds__(256) void k_search_table(Slam2dLidar lid, int nth, double th0, double dth, const double* __restrict__ ranges,
                                                      double2* __restrict__ E, unsigned long long* __restrict__ out, int positions) {
    const unsigned i = blockIdx.x * 256u + threadIdx.x;                           // (positions < 2^31: no wrap)
    const int B = lid.beams;
    if (i < (unsigned)positions) out[i] = ~0ull;
    if (i >= (unsigned)(nth * B)) return;
    const int it = (int)i / B, b = (int)i - it * B;
    const double r = ranges[b];
    if (!(r < lid.max_range)) return;                                            // :84 (NaN and +inf are out, 0 and negatives in)
    int k = 0;
    for (int j = 0; j < b; ++j) k += ranges[j] < lid.max_range;
    const double th = th0 + (double)it * dth;
    const double a = fan_of(lid, th).angle(b);
    E[(size_t)it * B + k] = make_double2(cos(a) * r, sin(a) * r);                // :87-88
}

// The cost of the pose at (x, y) whose heading's endpoint offsets are e[0 .. n_rng): slam2d_search_lattice's cost, for its search
// launch and slam2d_refine_poses'.  The lane sums the inside beams' costs and counts them in registers -- a beam that is not
// inside loads cell 0 of the image and adds nothing: no branch in the loop, so the gathers of SEARCH_UNROLL beams are in flight
// together (the table entries first: one wait for all of them).  n_rng is the same for every lane of the wave.
__device__ __forceinline__ unsigned long long offsets_cost(const double2* __restrict__ e, const int n_rng, const double x, const double y,
                                                           const Slam2dFrame& fr, const double step, const FieldSize fs, const int fpitch,
                                                           const uint32_t* __restrict__ field, const unsigned outside_cost) {
    unsigned long long sum_b = 0ull;
    int n_in = 0;
    const auto beam = [&](const double2 d) {
        int cx, cy;
        const bool inside = score_cell(x + d.x, y + d.y, fr.xlo, fr.ylo, step, fs.fw, fs.fh, cx, cy);
        const uint32_t cost = field[inside ? cy * fpitch + cx : 0];              // (fmax * fpitch < 2^29)
        sum_b += inside ? cost : 0u;
        n_in += inside;
    };
    int k = 0;
    for (; k + SEARCH_UNROLL <= n_rng; k += SEARCH_UNROLL) {
        double2 d[SEARCH_UNROLL];
#pragma unroll
        for (int u = 0; u < SEARCH_UNROLL; ++u) d[u] = e[k + u];
#pragma unroll
        for (int u = 0; u < SEARCH_UNROLL; ++u) beam(d[u]);
    }
    for (; k < n_rng; ++k) beam(e[k]);
    return sum_b + (unsigned long long)(n_rng - n_in) * outside_cost;
}

// Position p of the lattice (flat index iy * nx + ix), headings [it0, it1) of this block row: both search launches' thread.  E's
// rows lie `pitch` entries apart and hold `count` offsets each.  The loops over headings and offsets are the same for every lane
// and E is read at a wave-uniform address.  The lane takes a heading's cost from offsets_cost, folds cost << 16 | it into a
// 64-bit minimum and joins the block rows with one integer atomicMin on d_out, which the table launch set to all ones in front of
// this launch on the same stream: a minimum of integers, whatever the order.
__device__ __forceinline__ void lattice_position(const unsigned p, const int nx, const int nth, const int hc, const double x0, const double dx,
                                                 const double y0, const double dy, const double2* __restrict__ E, const int pitch, const int count,
                                                 const Slam2dLevel& lv, const SlotField& sf, const unsigned outside_cost,
                                                 unsigned long long* __restrict__ out) {
    const int iy = (int)p / nx, ix = (int)p - iy * nx;
    const double x = x0 + (double)ix * dx, y = y0 + (double)iy * dy;
    const int it0 = blockIdx.y * hc, it1 = min(nth, it0 + hc);
    unsigned long long best = ~0ull;
    for (int it = it0; it < it1; ++it) {
        const unsigned long long cost = offsets_cost(E + (size_t)it * pitch, count, x, y, sf.fr, lv.step, sf.fs, lv.fpitch, sf.field, outside_cost);
        best = min(best, (cost << 16) | (unsigned long long)it);
    }
    atomicMin(&out[p], best);
}

// Search launch: one thread per position (neighbouring lanes read neighbouring field cells), blockIdx.y takes headings
// [y * hc, y * hc + hc): lattice_position with the beams in range counted (the same at every pose; the lanes of a wave read
// ranges[b] at one address).  Reads frames[p_field], the slot's field, E and the ranges; no fault bit.
__global__ __launch_bounds__(256) void k_search_lattice(Slam2dLidar lid, Slam2dLevel lv, int p_field, int nx, int positions, int nth, int hc,
                                                        double x0, double dx, double y0, double dy, const double* __restrict__ ranges,
                                                        const double2* __restrict__ E, unsigned outside_cost,
                                                        unsigned long long* __restrict__ out) {
    const unsigned p = blockIdx.x * 256u + threadIdx.x;                           // (positions < 2^31: no wrap)
    if (p >= (unsigned)positions) return;
    const SlotField sf = slot_field(lv, p_field);
    const int B = lid.beams;
    int n_rng = 0;                                                               // beams in range: the same at every pose
    for (int b = 0; b < B; ++b) n_rng += ranges[b] < lid.max_range;
    lattice_position(p, nx, nth, hc, x0, dx, y0, dy, E, B, n_rng, lv, sf, outside_cost, out);
}

// ---- a local search around each of N seed poses (slam2d_refine_poses) ----
#define REFINE_TABLE 2048            // endpoint offsets (16 B each) of one block's LDS table: a block row takes at most REFINE_TABLE / beams headings, at least one
#define REFINE_BLOCKS 1024           // blocks that fill the card (256 CUs x 4): with fewer seeds a seed's headings are split over block rows

// the centre-first order of an axis: 0, +1, -1, +2, -2, ...
__host__ __device__ __forceinline__ int refine_off(const int j) { return ((j + 1) >> 1) * ((j & 1) ? 1 : -1); }

struct RefineLattice { int nx, ny, nth; double dx, dy, dth; };

// headings per block row: all of them where the seeds alone fill the card, fewer -- down to one -- where they do not, and never
// more than the LDS table holds
static int refine_chunk(const int N, const int nth, const int beams) {
    const int fit = REFINE_TABLE / beams > 1 ? REFINE_TABLE / beams : 1;
    const long long rows = (REFINE_BLOCKS + (long long)N - 1) / N;                // block rows wanted per seed (>= 1)
    const long long hc = ((long long)nth + rows - 1) / rows;
    return hc < fit ? (int)hc : fit;
}

__device__ __forceinline__ unsigned long long wave64_min_u64(unsigned long long v) {            // (all 64 lanes active)
    v = min(v, dpp_u64<0xB1>(v)); v = min(v, dpp_u64<0x4E>(v)); v = min(v, dpp_u64<0x141>(v)); v = min(v, dpp_u64<0x140>(v));
    unsigned long long m = ~0ull;
#pragma unroll
    for (int l = 0; l < 64; l += 16)
        m = min(m, ((unsigned long long)(unsigned)__builtin_amdgcn_readlane((int)(unsigned)(v >> 32), l) << 32) |
                       (unsigned)__builtin_amdgcn_readlane((int)(unsigned)v, l));
    return m;
}

// First launch, one thread per seed: the move (mcl_move_particle's, without noise; no motion: the seed's bits) into moved[n][3], and
// the identity of the search launch's atomicMin into out[2 n].
__global__ __launch_bounds__(256) void k_refine_move(int N, const double* __restrict__ pose, int pstride, int has_motion, double dfwd, double dside,
                                                     double dturn, double* __restrict__ moved, unsigned long long* __restrict__ out) {
    const int n = blockIdx.x * 256 + threadIdx.x;
    if (n >= N) return;
    const double x = pose[(size_t)n * pstride], y = pose[(size_t)n * pstride + 1], th = pose[(size_t)n * pstride + 2];
    double* m = moved + (size_t)n * 3;
    if (has_motion) {
        const double c = cos(th), s = sin(th);
        m[0] = (x + c * dfwd) - s * dside;
        m[1] = (y + s * dfwd) + c * dside;
        m[2] = th + dturn;
    } else {
        m[0] = x; m[1] = y; m[2] = th;
    }
    out[(size_t)n * SLAM2D_REFINE_STRIDE] = ~0ull;
}

// The block's share of a compaction in item order (beams, points): whether this thread's item is kept -> its slot; `total` runs on, the same in
// every thread.  Ballots for a wave's count, the four waves' counts through LDS; both barriers are the block's.
__device__ __forceinline__ int block_compact_slot(const bool keep, int* wcount, const int wv, const int lane, int& total) {
    const unsigned long long mask = __ballot(keep);
    if (lane == 0) wcount[wv] = __popcll(mask);
    __syncthreads();
    int base = total;
#pragma unroll
    for (int w = 0; w < 4; ++w) {
        const int c = wcount[w];
        if (w < wv) base += c;
        total += c;
    }
    __syncthreads();
    return base + __popcll(mask & ((1ull << lane) - 1ull));
}

// What a block of the two refinement searches is given: blockIdx.x = n * rows + row takes headings [jt0, jt0 + hn) of seed n, whose
// moved pose is (xm, ym, tm)
struct RefineBlock { int n, jt0, hn; double xm, ym, tm; };
__device__ __forceinline__ RefineBlock refine_block(const int rows, const int hc, const RefineLattice& lat, const double* __restrict__ moved) {
    const int n = (int)(blockIdx.x / (unsigned)rows), row = (int)(blockIdx.x - (unsigned)n * (unsigned)rows);
    const int jt0 = row * hc;
    return RefineBlock{n, jt0, min(hc, lat.nth - jt0), moved[(size_t)n * 3], moved[(size_t)n * 3 + 1], moved[(size_t)n * 3 + 2]};
}

// The last phase of both refinement searches, behind the barrier that completes the block's table E[hn][count]: the block's
// candidates (h, jy, jx), jx fastest, over the threads -- neighbouring lanes are neighbouring jx of one heading, so their gathers
// fall on neighbouring field cells; every lane runs the same offset loop (offsets_cost).  cost << 20 | f is folded per thread and
// per wave and joins the block rows -- and a block's waves -- with a 64-bit integer atomicMin on out[2 n], which k_refine_move set
// to all ones: a minimum of integers, whatever the order.  The thread that holds f == 0 stores its cost in out[2 n + 1].
__device__ __forceinline__ void refine_candidates(const RefineBlock& rb, const RefineLattice& lat, const double2* E, const int count,
                                                  const Slam2dLevel& lv, const SlotField& sf, const unsigned outside_cost,
                                                  unsigned long long* __restrict__ out) {
    const int P = lat.nx * lat.ny, f0 = rb.jt0 * P;                              // (nx * ny * nth <= 2^20)
    unsigned long long best = ~0ull;
    for (int c = threadIdx.x; c < rb.hn * P; c += 256) {
        const int h = c / P, p = c - h * P, jy = p / lat.nx, jx = p - jy * lat.nx;
        const double x = rb.xm + (double)refine_off(jx) * lat.dx, y = rb.ym + (double)refine_off(jy) * lat.dy;
        const unsigned long long cost = offsets_cost(E + h * count, count, x, y, sf.fr, lv.step, sf.fs, lv.fpitch, sf.field, outside_cost);
        if (f0 + c == 0) out[(size_t)rb.n * SLAM2D_REFINE_STRIDE + 1] = cost;
        best = min(best, (cost << 20) | (unsigned long long)(f0 + c));
    }
    best = wave64_min_u64(best);
    if ((threadIdx.x & 63) == 0 && best != ~0ull) atomicMin(&out[(size_t)rb.n * SLAM2D_REFINE_STRIDE], best);
}

// Search launch: refine_block's headings of its seed (hc * beams <= REFINE_TABLE or hc == 1: slam2d_refine_poses).  Three
// phases, a barrier between them:
//   1. the scan's beams IN RANGE, compacted in beam order into bidx (block_compact_slot);
//   2. E[h][k] = (cos(a) * r, sin(a) * r) of the block's heading h and the k-th beam in range -- the only cos / sin of the search:
//      a heading's are evaluated once per seed, not once per candidate; the products rounded here so that x + e is x + cos(a) * r;
//   3. refine_candidates.
// Reads frames[p_field], the slot's field, the moved seeds and the ranges; no fault bit.
__global__ __launch_bounds__(256) void k_refine_search(Slam2dLidar lid, Slam2dLevel lv, int p_field, int rows, int hc, RefineLattice lat,
                                                       const double* __restrict__ moved, const double* __restrict__ ranges, int rstride,
                                                       unsigned outside_cost, unsigned long long* __restrict__ out) {
    __shared__ double2 E[REFINE_TABLE];
    __shared__ unsigned short bidx[SLAM2D_MAX_BEAMS];
    __shared__ int wcount[4];
    const int tid = threadIdx.x, wv = tid >> 6, lane = tid & 63;
    const RefineBlock rb = refine_block(rows, hc, lat, moved);
    const SlotField sf = slot_field(lv, p_field);
    const double* __restrict__ rg = ranges + (size_t)rb.n * rstride;
    const int B = lid.beams;
    int n_rng = 0;                                                               // beams in range (block-uniform)
    for (int b0 = 0; b0 < B; b0 += 256) {
        const int b = b0 + tid;
        const bool in_range = b < B && rg[b] < lid.max_range;                    // :84 (NaN and +inf are out, 0 and negatives in)
        const int slot = block_compact_slot(in_range, wcount, wv, lane, n_rng);
        if (in_range) bidx[slot] = (unsigned short)b;
    }
    __syncthreads();
    for (int i = tid; i < rb.hn * n_rng; i += 256) {                             // (hn * n_rng <= REFINE_TABLE)
        const int h = i / n_rng, b = bidx[i - h * n_rng];
        const double r = rg[b];
        const double a = fan_of(lid, rb.tm + (double)refine_off(rb.jt0 + h) * lat.dth).angle(b);
        E[i] = make_double2(cos(a) * r, sin(a) * r);                             // :87-88
    }
    __syncthreads();
    refine_candidates(rb, lat, E, n_rng, lv, sf, outside_cost, out);
}

// Last launch, one thread per seed: the winning candidate's pose from its flat index, by the candidates' own three operations
__global__ __launch_bounds__(256) void k_refine_pose(int N, RefineLattice lat, const double* __restrict__ moved,
                                                     const unsigned long long* __restrict__ out, double* __restrict__ pose, int pstride) {
    const int n = blockIdx.x * 256 + threadIdx.x;
    if (n >= N) return;
    const int f = (int)(out[(size_t)n * SLAM2D_REFINE_STRIDE] & 0xfffffull);
    const int P = lat.nx * lat.ny, jt = f / P, p = f - jt * P, jy = p / lat.nx, jx = p - jy * lat.nx;
    double* o = pose + (size_t)n * pstride;
    o[0] = moved[(size_t)n * 3] + (double)refine_off(jx) * lat.dx;
    o[1] = moved[(size_t)n * 3 + 1] + (double)refine_off(jy) * lat.dy;
    o[2] = moved[(size_t)n * 3 + 2] + (double)refine_off(jt) * lat.dth;
}

// ---- the local search with a charge per beam that crosses a wall (slam2d_refine_poses_rays) ----
// COST with slam2d_score_rays' THROUGH beams on a stride of the scan: the endpoint part of a candidate is offsets_cost on
// k_refine_search's table, the ray pass behind it is ray_walk.  The move launch is k_refine_move; the search and the last launch
// are this section's.
#define REFINE_RAYS_WAVES 4          // seeds (waves) per block of the last launch

// The CAST beams, the margin and the charge of a refinement
struct RefineRays { int stride, phase, margin; unsigned through_cost; };

// CHECKED and kend of a beam in range, k_score_rays' lines: -1 where the beam is not checked (never THROUGH, as kend < 0)
__device__ __forceinline__ long long refine_ray_kend(const double r, const double step, const int margin) {
    const double q = r / step;
    return q >= 0.0 && q < 1e9 ? (long long)q - margin : -1ll;
}

// J, the number of CAST beams: phase + (J - 1) * stride <= B - 1
__host__ __device__ __forceinline__ int refine_rays_cast(const int B, const int stride, const int phase) {
    return phase < B ? (B - 1 - phase) / stride + 1 : 0;
}
// The search block's dynamic LDS: E[hc][B] and U[hc][J] of 16 bytes, kend_s[J] of 4, bidx[B] and kslot[B] of 2 -- 40 KB at 180
// beams, stride 4 and the most headings a row takes (11), at most 80 KiB (2048 beams, stride 1)
static size_t refine_rays_lds_bytes(const int hc, const int B, const int J) { return 16 * (size_t)hc * (B + J) + 4 * (size_t)(B + J); }

// Search launch: k_refine_search's block and headings per block row (the same hc: the second table enlarges the block's LDS,
// which is dynamic so that a block asks for what its beams need and several share a CU), its phases with three things more:
//   1. beside the beams IN RANGE (bidx), the KEPT ones among them -- CAST, CHECKED and kend >= 0: the others are never THROUGH,
//      whatever the pose --, compacted in beam order: kslot[k] = the kept slot of the k-th beam in range (NO_SLOT: not kept),
//      kend_s[j] = kend of the j-th kept beam;
//   2. with E[h][k], U[h][j] = (cos(a), sin(a)) of heading h and the j-th kept beam: ONE evaluation of cos / sin gives both (E's
//      rounded products cannot give them back);
//   3. the candidates, jx fastest over the threads as in refine_candidates, in WHOLE waves: ray_walk is a ballot loop, so a lane
//      behind the last candidate runs every trip with active = false (it walks nothing and costs nothing).  A lane's endpoint cost
//      is offsets_cost; then the kept beams in turn, one ray_walk per beam for the wave -- its lanes are neighbouring positions of
//      (mostly) one heading: parallel rays about a cell apart, of one length, whose gathers fall on neighbouring cells.  A
//      non-finite candidate is LEFT at 0 on every beam.  cost << 20 | f is joined as in refine_candidates; the thread that holds
//      f == 0 stores its charged cost in out[2 n + 1].
// Every ray ends: ray_walk's k strictly increases below kend + 1 < 2^30.  Reads frames[p_field], the slot's field and squared
// distances, the moved seeds and the ranges; no fault bit.
#define REFINE_NO_SLOT 0xffffu
__global__ __launch_bounds__(256) void k_refine_search_rays(Slam2dLidar lid, Slam2dLevel lv, int p_field, const uint32_t* __restrict__ dist2, int rows,
                                                            int hc, RefineLattice lat, const double* __restrict__ moved,
                                                            const double* __restrict__ ranges, int rstride, unsigned outside_cost, RefineRays ry,
                                                            unsigned long long* __restrict__ out) {
    extern __shared__ __attribute__((aligned(16))) unsigned char refine_rays_lds[];     // refine_rays_lds_bytes(hc, B, J)
    __shared__ int wcount[4];
    const int tid = threadIdx.x, wv = tid >> 6, lane = tid & 63;
    const RefineBlock rb = refine_block(rows, hc, lat, moved);
    const SlotField sf = slot_field(lv, p_field);
    const RayField f = ray_field(lv, p_field, dist2);
    const double* __restrict__ rg = ranges + (size_t)rb.n * rstride;
    const int B = lid.beams, J = refine_rays_cast(B, ry.stride, ry.phase);
    double2* E = reinterpret_cast<double2*>(refine_rays_lds);                    // [hc][B]: hn * n_rng in use
    double2* U = E + (size_t)hc * B;                                             // [hc][J]: hn * n_kept in use
    int* kend_s = reinterpret_cast<int*>(U + (size_t)hc * J);                    // [J]
    unsigned short* bidx = reinterpret_cast<unsigned short*>(kend_s + J);        // [B]
    unsigned short* kslot = bidx + B;                                            // [B]
    int n_rng = 0, n_kept = 0;                                                   // beams in range, kept beams (block-uniform)
    for (int b0 = 0; b0 < B; b0 += 256) {
        const int b = b0 + tid;
        const double r = b < B ? rg[b] : NAN;
        const bool in_range = r < lid.max_range;                                 // :84 (NaN and +inf are out, 0 and negatives in)
        const long long kend = in_range && b % ry.stride == ry.phase ? refine_ray_kend(r, lv.step, ry.margin) : -1ll;
        const int slot = block_compact_slot(in_range, wcount, wv, lane, n_rng);
        const int kept = block_compact_slot(kend >= 0, wcount, wv, lane, n_kept);
        if (in_range) {
            bidx[slot] = (unsigned short)b;
            kslot[slot] = kend >= 0 ? (unsigned short)kept : (unsigned short)REFINE_NO_SLOT;
        }
        if (kend >= 0) kend_s[kept] = (int)kend;                                 // (below 1e9)
    }
    __syncthreads();
    for (int i = tid; i < rb.hn * n_rng; i += 256) {                             // (hn * n_rng <= REFINE_TABLE)
        const int h = i / n_rng, k = i - h * n_rng, b = bidx[k];
        const double r = rg[b];
        const double a = fan_of(lid, rb.tm + (double)refine_off(rb.jt0 + h) * lat.dth).angle(b);
        const double c = cos(a), s = sin(a);
        E[i] = make_double2(c * r, s * r);                                       // :87-88
        const unsigned j = kslot[k];
        if (j != REFINE_NO_SLOT) U[h * n_kept + (int)j] = make_double2(c, s);
    }
    __syncthreads();
    const int P = lat.nx * lat.ny, f0 = rb.jt0 * P, total = rb.hn * P;           // (nx * ny * nth <= 2^20)
    unsigned long long best = ~0ull;
    for (int c0 = 0; c0 < total; c0 += 256) {                                    // (block-uniform: whole waves reach ray_walk)
        const int c = c0 + tid;
        const bool active = c < total;
        const int h = active ? c / P : 0, p = active ? c - h * P : 0, jy = p / lat.nx, jx = p - jy * lat.nx;
        const double x = rb.xm + (double)refine_off(jx) * lat.dx, y = rb.ym + (double)refine_off(jy) * lat.dy;
        unsigned long long cost = 0ull;
        if (active) cost = offsets_cost(E + h * n_rng, n_rng, x, y, sf.fr, lv.step, sf.fs, lv.fpitch, sf.field, outside_cost);
        const double2* __restrict__ u = U + h * n_kept;
        int thr = 0;
        for (int j = 0; j < n_kept; ++j) {                                       // (block-uniform)
            const double2 d = u[j];
            const uint32_t word = ray_walk(f, x, y, d.x, d.y, kend_s[j], active);
            thr += active && (word >> 30) == SLAM2D_RAY_HIT;                      // (a HIT lies at k <= the limit, kend)
        }
        if (active) {
            cost += (unsigned long long)thr * ry.through_cost;                   // (below 2^44: two terms of at most 2^43)
            if (f0 + c == 0) out[(size_t)rb.n * SLAM2D_REFINE_STRIDE + 1] = cost;
            best = min(best, (cost << 20) | (unsigned long long)(f0 + c));
        }
    }
    best = wave64_min_u64(best);
    if (lane == 0 && best != ~0ull) atomicMin(&out[(size_t)rb.n * SLAM2D_REFINE_STRIDE], best);
}

// Last launch, a wave per seed: k_refine_pose's winning pose -- every lane forms it, lane 0 stores it --, then that pose's CAST
// beams packed over the lanes as in mcl_score_rays_particle, 64 rays a trip: a_b, cos and sin by the search's own expressions on
// the same th', so the rays are the searching thread's bit for bit and through[n] is the count inside the winning word.
__global__ __launch_bounds__(64 * REFINE_RAYS_WAVES) void k_refine_pose_rays(Slam2dLidar lid, Slam2dLevel lv, int p_field,
                                                                            const uint32_t* __restrict__ dist2, int N, RefineLattice lat,
                                                                            const double* __restrict__ moved, const double* __restrict__ ranges,
                                                                            int rstride, RefineRays ry, const unsigned long long* __restrict__ out,
                                                                            double* __restrict__ pose, int pstride, uint32_t* __restrict__ through) {
    const int lane = threadIdx.x & 63;
    const int n = blockIdx.x * REFINE_RAYS_WAVES + (threadIdx.x >> 6);
    if (n >= N) return;                                                          // (wave-uniform)
    const int fi = (int)(out[(size_t)n * SLAM2D_REFINE_STRIDE] & 0xfffffull);
    const int P = lat.nx * lat.ny, jt = fi / P, p = fi - jt * P, jy = p / lat.nx, jx = p - jy * lat.nx;
    const double x = moved[(size_t)n * 3] + (double)refine_off(jx) * lat.dx;
    const double y = moved[(size_t)n * 3 + 1] + (double)refine_off(jy) * lat.dy;
    const double th = moved[(size_t)n * 3 + 2] + (double)refine_off(jt) * lat.dth;
    if (lane == 0) {
        double* o = pose + (size_t)n * pstride;
        o[0] = x; o[1] = y; o[2] = th;
    }
    const RayField f = ray_field(lv, p_field, dist2);
    const double* __restrict__ rg = ranges + (size_t)n * rstride;
    const int B = lid.beams;
    const BeamFan fan = fan_of(lid, th);
    const int J = refine_rays_cast(B, ry.stride, ry.phase);
    int n_thr = 0;
    for (int j0 = 0; j0 < J; j0 += 64) {                                         // (wave-uniform trip count)
        const bool cast = j0 + lane < J;
        const int b = cast ? ry.phase + (j0 + lane) * ry.stride : 0;
        const double r = cast ? rg[b] : NAN;
        const long long kend = r < lid.max_range ? refine_ray_kend(r, lv.step, ry.margin) : -1ll;
        const double a = fan.angle(b);
        const uint32_t word = ray_walk(f, x, y, cos(a), sin(a), kend >= 0 ? (int)kend : 0, kend >= 0);
        n_thr += __popcll(__ballot(kend >= 0 && (word >> 30) == SLAM2D_RAY_HIT));
    }
    if (lane == 0) through[n] = (uint32_t)n_thr;
}

// ---- the two searches for a set of points in the robot's frame (slam2d_search_points, slam2d_refine_points) ----
// The table is the only place where the searches look at their input: E[heading][k] = R(heading) q of the k-th VALID point q, and
// offsets_cost, the packed minima and the joins behind it are the scan forms'.  A heading costs ONE cos / sin, whatever M.
#define POINTS_HEADS 128             // headings whose cos / sin one pass of k_refine_points' table phase holds in LDS

// point k of a set is VALID iff both of its coordinates are finite (include/slam2d.h, step 1)
__device__ __forceinline__ bool point_valid(const double* __restrict__ pts, const int pstride, const int k) {
    return __builtin_isfinite(pts[(size_t)k * pstride]) && __builtin_isfinite(pts[(size_t)k * pstride + 1]);
}
// R(th) q from c = cos(th), s = sin(th): two rounded products and one rounded add or subtract per component (step 2)
__device__ __forceinline__ double2 point_offset(const double c, const double s, const double qx, const double qy) {
    return make_double2(c * qx - s * qy, s * qx + c * qy);
}
// First launch of the search: block `it` < nth writes heading it's row E[it][0 .. valid) -- thread 0 evaluates the heading's cos /
// sin, the only ones of the search, the block compacts the valid points in point order and rotates them -- and every block sets
// its 256 words of d_out to all ones, the identity of the search launch's atomicMin (the grid covers both: slam2d_search_points).
__global__ __launch_bounds__(256) void k_points_table(int nth, double th0, double dth, const double* __restrict__ pts, int pstride, int M,
                                                      double2* __restrict__ E, unsigned long long* __restrict__ out, int positions) {
    __shared__ double2 cs;
    __shared__ int wcount[4];
    const int tid = threadIdx.x, wv = tid >> 6, lane = tid & 63;
    const unsigned i = blockIdx.x * 256u + threadIdx.x;                           // (positions < 2^31: no wrap)
    if (i < (unsigned)positions) out[i] = ~0ull;
    if (blockIdx.x >= (unsigned)nth) return;                                     // (block-uniform)
    const int it = (int)blockIdx.x;
    if (tid == 0) {
        const double th = th0 + (double)it * dth;
        cs = make_double2(cos(th), sin(th));
    }
    __syncthreads();
    const double c = cs.x, s = cs.y;
    double2* __restrict__ row = E + (size_t)it * M;
    int valid = 0;
    for (int k0 = 0; k0 < M; k0 += 256) {
        const int k = k0 + tid;
        const bool keep = k < M && point_valid(pts, pstride, k);
        const int slot = block_compact_slot(keep, wcount, wv, lane, valid);
        if (keep) row[slot] = point_offset(c, s, pts[(size_t)k * pstride], pts[(size_t)k * pstride + 1]);
    }
}

// Search launch: k_search_lattice's, lattice_position with the valid points counted in place of the beams in range (the same at
// every pose; the lanes of a wave read a point at one address).  Reads frames[p_field], the slot's field, E and the points; no
// fault bit.
__global__ __launch_bounds__(256) void k_points_lattice(Slam2dLevel lv, int p_field, int nx, int positions, int nth, int hc, double x0, double dx,
                                                        double y0, double dy, const double* __restrict__ pts, int pstride, int M,
                                                        const double2* __restrict__ E, unsigned outside_cost,
                                                        unsigned long long* __restrict__ out) {
    const unsigned p = blockIdx.x * 256u + threadIdx.x;                           // (positions < 2^31: no wrap)
    if (p >= (unsigned)positions) return;
    const SlotField sf = slot_field(lv, p_field);
    int valid = 0;
    for (int k = 0; k < M; ++k) valid += point_valid(pts, pstride, k);
    lattice_position(p, nx, nth, hc, x0, dx, y0, dy, E, M, valid, lv, sf, outside_cost, out);
}

// Search launch of the refinement: k_refine_search's block (hc * M <= REFINE_TABLE or hc == 1) with the first two phases for points:
//   1. the set's VALID points, compacted in point order into kidx;
//   2. E[h][k] = R(tm + off(jt0 + h) * dth) q of the block's heading h and the k-th valid point q: the headings' cos / sin first,
//      one per heading and seed and POINTS_HEADS of them at a time, then the rotations;
//   3. refine_candidates.
// Reads frames[p_field], the slot's field, the moved seeds and the points; no fault bit.
__global__ __launch_bounds__(256) void k_refine_points(Slam2dLevel lv, int p_field, int rows, int hc, RefineLattice lat,
                                                       const double* __restrict__ moved, const double* __restrict__ points, int pstride, int M,
                                                       int sstride, unsigned outside_cost, unsigned long long* __restrict__ out) {
    __shared__ double2 E[REFINE_TABLE];
    __shared__ double2 cs[POINTS_HEADS];
    __shared__ unsigned short kidx[SLAM2D_MAX_POINTS];
    __shared__ int wcount[4];
    const int tid = threadIdx.x, wv = tid >> 6, lane = tid & 63;
    const RefineBlock rb = refine_block(rows, hc, lat, moved);
    const SlotField sf = slot_field(lv, p_field);
    const double* __restrict__ pts = points + (size_t)rb.n * sstride;
    int valid = 0;                                                               // (block-uniform)
    for (int k0 = 0; k0 < M; k0 += 256) {
        const int k = k0 + tid;
        const bool keep = k < M && point_valid(pts, pstride, k);
        const int slot = block_compact_slot(keep, wcount, wv, lane, valid);
        if (keep) kidx[slot] = (unsigned short)k;
    }
    __syncthreads();
    for (int h0 = 0; h0 < rb.hn; h0 += POINTS_HEADS) {                           // (one pass from 16 points on: hn * valid <= REFINE_TABLE)
        const int h1 = min(rb.hn, h0 + POINTS_HEADS);
        if (tid < h1 - h0) {
            const double th = rb.tm + (double)refine_off(rb.jt0 + h0 + tid) * lat.dth;
            cs[tid] = make_double2(cos(th), sin(th));
        }
        __syncthreads();
        for (int i = h0 * valid + tid; i < h1 * valid; i += 256) {
            const int h = i / valid, k = kidx[i - h * valid];
            E[i] = point_offset(cs[h - h0].x, cs[h - h0].y, pts[(size_t)k * pstride], pts[(size_t)k * pstride + 1]);
        }
        __syncthreads();
    }
    refine_candidates(rb, lat, E, valid, lv, sf, outside_cost, out);
}

// slam2d_score_points: k_score_poses' wave per pose and its hash set of cell keys (hsize = score_hash_size(M)), with R(theta) q
// of the pose's set for an endpoint -- points interleaved over the lanes (point = 64 i + lane), one cos / sin per pose, which
// every lane of the wave evaluates alike.  Slot 4 is the number of VALID points.  Reads frames[p_field], the slot's field and the
// inputs; writes out; no global atomic, no fault bit.
__global__ __launch_bounds__(64 * SCORE_WAVES) void k_score_points(Slam2dLevel lv, int p_field, int N, int hsize, const double* __restrict__ pose,
                                                                   int pstride, const double* __restrict__ points, int ptstride, int M, int sstride,
                                                                   double* __restrict__ out) {
    extern __shared__ __attribute__((aligned(16))) int score_lds[];              // [blockDim.x / 64][hsize] keys
    const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int n = blockIdx.x * (blockDim.x >> 6) + wv;
    int* hkey = score_lds + wv * hsize;
    const int hmask = hsize - 1;
    for (int i = lane; i < hsize; i += 64) hkey[i] = INT_MAX;                    // (no key: cx < 2^15 leaves the low half below 0xffff)
    __syncthreads();
    if (n >= N) return;                                                          // (wave-uniform)
    const SlotField sf = slot_field(lv, p_field);
    const double x = pose[(size_t)n * pstride], y = pose[(size_t)n * pstride + 1], th = pose[(size_t)n * pstride + 2];
    const double c = cos(th), s = sin(th);
    const double* __restrict__ pts = points + (size_t)n * sstride;
    unsigned long long sum_u = 0ull, sum_b = 0ull;                               // (this lane's share)
    int n_u = 0, n_in = 0, n_val = 0;                                            // (the wave's counts: ballots)
    for (int k0 = 0; k0 < M; k0 += 64) {                                         // (wave-uniform trip count)
        const int k = k0 + lane;
        const bool valid = k < M && point_valid(pts, ptstride, k);
        bool inside = false;
        int key = INT_MAX;
        uint32_t cost = 0u;
        if (valid) {
            const double2 e = point_offset(c, s, pts[(size_t)k * ptstride], pts[(size_t)k * ptstride + 1]);
            int cx, cy;
            if (score_cell(x + e.x, y + e.y, sf.fr.xlo, sf.fr.ylo, lv.step, sf.fs.fw, sf.fs.fh, cx, cy)) {
                inside = true;
                key = (cy << 16) | cx;
                cost = sf.field[(size_t)cy * lv.fpitch + cx];
            }
        }
        bool owns = false;
        if (inside) {
            int slot;
            owns = cell_set_insert(hkey, hmask, key, slot);
            sum_b += cost;
            if (owns) sum_u += cost;
        }
        n_val += __popcll(__ballot(valid));
        n_in += __popcll(__ballot(inside));
        n_u += __popcll(__ballot(owns));
    }
    sum_u = wave64_sum_u64(sum_u);
    sum_b = wave64_sum_u64(sum_b);
    if (lane == 0) {
        const double inv = 1.0 / lv.cost_scale;
        double* o = out + (size_t)n * SLAM2D_SCORE_STRIDE;
        o[0] = -((double)sum_u * inv); o[1] = (double)n_u; o[2] = -((double)sum_b * inv); o[3] = (double)n_in;
        o[4] = (double)n_val; o[5] = (double)sum_u; o[6] = (double)sum_b; o[7] = 0.0;
    }
}

// ---- Monte-Carlo localisation in a known map (slam2d_mcl_step): move, weigh, resample, all in integers and rounded operations ----
#define MCL_WAVES 4                  // particles (waves) per block of the scoring launch
#define MCL_UNROLL 2                 // trips of 64 beams its beam loop takes at a time: their gathers are in flight together
#define MCL_SCAN_BLOCK 1024          // particles one block of the scan launch covers, 4 per thread (tests/test_gpu_mcl.py names it)
#define MCL_TAIL 8                   // words of d_work behind its arrays: the packed minimum, then padding

// d_work of slam2d_mcl_step: the moved poses [N][3], the costs [N], the weights' block-local prefix sums [N], the scan blocks'
// sums (then: their exclusive prefix sums) [MCL_SCAN_BLOCK -- at most that many blocks at SLAM2D_MCL_MAX_PARTICLES], the tail
struct MclWork {
    double* moved;
    unsigned long long *cost, *csum, *bsum, *key;
};
__host__ __device__ __forceinline__ long long mcl_work_words(const int N) { return 5ll * N + MCL_SCAN_BLOCK + MCL_TAIL; }
__host__ __device__ __forceinline__ MclWork mcl_work_of(uint64_t* w, const int N) {
    unsigned long long* u = (unsigned long long*)w;
    return MclWork{reinterpret_cast<double*>(w), u + 3ll * N, u + 4ll * N, u + 5ll * N, u + 5ll * N + MCL_SCAN_BLOCK};
}

// Philox4x32-10 (Salmon, Moraes, Dror, Shaw 2011): ten rounds, the key bumped behind each
struct Philox4 { uint32_t v[4]; };
__device__ __forceinline__ Philox4 philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1) {
#pragma unroll
    for (int i = 0; i < 10; ++i) {
        const unsigned long long p0 = 0xD2511F53ull * c0, p1 = 0xCD9E8D57ull * c2;
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
        c0 = n0; c1 = (uint32_t)p1; c2 = n2; c3 = (uint32_t)p0;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
    return Philox4{{c0, c1, c2, c3}};
}
// draw j of particle n: the four words as int32 summed, times 2^-31 -- exact, |g| < 4, Irwin-Hall of four (variance 4/3)
__device__ __forceinline__ double mcl_noise(const uint32_t n, const uint32_t j, const uint64_t seed, const uint64_t scan) {
    const Philox4 o = philox4x32_10(n, j, (uint32_t)scan, (uint32_t)(scan >> 32), (uint32_t)seed, (uint32_t)(seed >> 32));
    const long long S = (long long)(int32_t)o.v[0] + (int32_t)o.v[1] + (int32_t)o.v[2] + (int32_t)o.v[3];
    return (double)S * 0x1p-31;
}

// Inclusive prefix sum of v over the block's threads in thread order (blockDim.x a multiple of 64, at most 1024); total: the
// block's sum.  lds: 16 words.  Integers: the same bits whatever the order of arrival.
__device__ __forceinline__ unsigned long long block_scan_u64(unsigned long long v, unsigned long long* lds, unsigned long long& total) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, nw = blockDim.x >> 6;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const unsigned long long u = __shfl_up(v, d, 64);
        if (lane >= d) v += u;
    }
    if (lane == 63) lds[wv] = v;
    __syncthreads();
    unsigned long long off = 0ull, tot = 0ull;
    for (int i = 0; i < nw; ++i) {
        const unsigned long long s = lds[i];
        if (i < wv) off += s;
        tot += s;
    }
    total = tot;
    return v + off;
}

// The identities of what the later launches of a step join with integer atomics: the packed minimum and the report's words 3,
// 6 and 10-14.  One thread of the first launch.
__device__ __forceinline__ void mcl_reset_joined(const MclWork& wk, unsigned long long* __restrict__ report) {
    *wk.key = ~0ull;
    report[3] = 0ull; report[6] = 0ull;
    for (int i = 10; i < 15; ++i) report[i] = 0ull;
}
// Particle n's three draws and its move, in the header's operations and order; returns the moved heading
__device__ __forceinline__ double mcl_move_particle(const int n, const double* __restrict__ pose, const int pstride, const double dfwd, const double dside,
                                                  const double dturn, const double amp0, const double amp1, const double amp2, const uint64_t seed,
                                                  const uint64_t scan, const MclWork& wk) {
    const double x0 = pose[(size_t)n * pstride], y0 = pose[(size_t)n * pstride + 1], th0 = pose[(size_t)n * pstride + 2];
    const double fx = dfwd + amp0 * mcl_noise((uint32_t)n, 0u, seed, scan), fy = dside + amp1 * mcl_noise((uint32_t)n, 1u, seed, scan);
    const double c = cos(th0), s = sin(th0);
    double* m = wk.moved + (size_t)n * 3;
    m[0] = (x0 + c * fx) - s * fy;
    m[1] = (y0 + s * fx) + c * fy;
    return m[2] = (th0 + dturn) + amp2 * mcl_noise((uint32_t)n, 2u, seed, scan);
}

// First launch, one thread per particle: mcl_move_particle; thread 0 also resets the joined words.  (Moving the pose inside the
// scoring launch, where a wave holds one particle, costs that wave a cos / sin of its own: as much as 64 beams, a fourth trip
// beside the three of 180 beams -- profiles/r13_mcl_step.md.)
__global__ __launch_bounds__(256) void k_mcl_move(int N, const double* __restrict__ pose, int pstride, double dfwd, double dside, double dturn,
                                                  double amp0, double amp1, double amp2, uint64_t seed, uint64_t scan, MclWork wk,
                                                  unsigned long long* __restrict__ report) {
    const int n = blockIdx.x * 256 + threadIdx.x;
    if (n == 0) mcl_reset_joined(wk, report);
    if (n >= N) return;
    mcl_move_particle(n, pose, pstride, dfwd, dside, dturn, amp0, amp1, amp2, seed, scan, wk);
}

// U trips of 64 beams of one particle, from beam b0: every cell first, then the gathers, then the sums.  A beam that is not inside
// -- out of range, beyond the last beam, outside the field, a quotient that fails the guard -- loads cell 0 of the image and adds
// nothing: no branch, so the U gathers are in flight together.
template <int U>
__device__ __forceinline__ void mcl_beams(const int b0, const int lane, const int B, const double* __restrict__ ranges, const double max_range,
                                          const BeamFan& fan, const double x, const double y, const Slam2dFrame& fr, const double step,
                                          const FieldSize fs, const int fpitch, const uint32_t* __restrict__ field,
                                          unsigned long long& sum_b, int& n_in, int& n_rng) {
    int idx[U];
    bool inside[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
        const int b = b0 + 64 * u + lane;
        const double r = b < B ? ranges[b] : NAN;
        const bool in_range = r < max_range;                                     // :84 (NaN and +inf are out, 0 and negatives in)
        const double a = fan.angle(b);
        const double px = x + cos(a) * r, py = y + sin(a) * r;                   // :87-88
        int cx, cy;
        inside[u] = score_cell(px, py, fr.xlo, fr.ylo, step, fs.fw, fs.fh, cx, cy) && in_range;
        idx[u] = inside[u] ? cy * fpitch + cx : 0;                               // (fmax * fpitch < 2^29)
        n_rng += __popcll(__ballot(in_range));
        n_in += __popcll(__ballot(inside[u]));
    }
    uint32_t cost[U];
#pragma unroll
    for (int u = 0; u < U; ++u) cost[u] = field[idx[u]];
#pragma unroll
    for (int u = 0; u < U; ++u) sum_b += inside[u] ? cost[u] : 0u;
}

// Particle n on this wave: k_score_poses' shape -- beams interleaved over the lanes, the ranges read contiguously -- without its
// cell set, on the moved pose; the trips of 64 beams go MCL_UNROLL at a time, the rest one by one.  cost << 20 | n joins the
// particles in one 64-bit integer atomicMin, sent only where it can lower the word as last read (a stale read costs an atomic,
// never the result).  Writes the particle's cost.
__device__ __forceinline__ void mcl_score_particle(const int n, const int lane, const Slam2dLidar& lid, const Slam2dLevel& lv, const Slam2dFrame& fr,
                                                   const FieldSize fs, const uint32_t* __restrict__ field, const double* __restrict__ ranges,
                                                   const unsigned outside_cost, const MclWork& wk) {
    const double x = wk.moved[(size_t)n * 3], y = wk.moved[(size_t)n * 3 + 1], th = wk.moved[(size_t)n * 3 + 2];
    const int B = lid.beams, trips = (B + 63) >> 6;
    const BeamFan fan = fan_of(lid, th);
    unsigned long long sum_b = 0ull;                                             // (this lane's share)
    int n_in = 0, n_rng = 0;                                                     // (the wave's counts: ballots)
    int t = 0;
    for (; t + MCL_UNROLL <= trips; t += MCL_UNROLL)                             // (wave-uniform trip counts)
        mcl_beams<MCL_UNROLL>(64 * t, lane, B, ranges, lid.max_range, fan, x, y, fr, lv.step, fs, lv.fpitch, field, sum_b, n_in, n_rng);
    for (; t < trips; ++t) mcl_beams<1>(64 * t, lane, B, ranges, lid.max_range, fan, x, y, fr, lv.step, fs, lv.fpitch, field, sum_b, n_in, n_rng);
    sum_b = wave64_sum_u64(sum_b);
    if (lane == 0) {
        const unsigned long long cost = sum_b + (unsigned long long)(n_rng - n_in) * outside_cost;      // (below 2^44 at 2048 beams)
        wk.cost[n] = cost;
        const unsigned long long v = (cost << 20) | (unsigned long long)n;
        if (v < __hip_atomic_load(wk.key, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMin(wk.key, v);
    }
}

// Score: one wave per particle (mcl_score_particle).  Reads frames[p_field], the slot's field, the moved poses and the ranges;
// writes the costs; no fault bit.
__global__ __launch_bounds__(64 * MCL_WAVES) void k_mcl_score(Slam2dLidar lid, Slam2dLevel lv, int p_field, int N, const double* __restrict__ ranges,
                                                              unsigned outside_cost, MclWork wk) {
    const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int n = blockIdx.x * MCL_WAVES + wv;
    if (n >= N) return;                                                          // (wave-uniform)
    const SlotField sf = slot_field(lv, p_field);
    mcl_score_particle(n, lane, lid, lv, sf.fr, sf.fs, sf.field, ranges, outside_cost, wk);
}

// Weigh and scan, a block of MCL_SCAN_BLOCK / 4 threads: block b takes particles [b * MCL_SCAN_BLOCK, ...) below N, four
// consecutive ones per thread; their integer weights from the table, the block-local inclusive prefix sums into csum, the block's
// sum into bsum[b], the weights above zero counted.  Every thread of the block calls it: the barriers are the block's.
__device__ __forceinline__ void mcl_weigh_block(const int N, const uint32_t* __restrict__ lut, const int lut_n, const int lut_shift, const MclWork& wk,
                                                unsigned long long* __restrict__ report) {
    __shared__ unsigned long long lds[16];
    __shared__ unsigned n_pos;
    if (threadIdx.x == 0) n_pos = 0u;
    const unsigned long long cmin = *wk.key >> 20;
    const int n0 = blockIdx.x * MCL_SCAN_BLOCK + threadIdx.x * 4;
    unsigned long long pre[4], run = 0ull;
    unsigned pos = 0u;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        uint32_t w = 0u;
        if (n0 + i < N) {
            const unsigned long long d = (wk.cost[n0 + i] - cmin) >> lut_shift;
            w = min(lut[d < (unsigned long long)(lut_n - 1) ? (int)d : lut_n - 1], (uint32_t)SLAM2D_MCL_MAX_WEIGHT);
        }
        pos += w > 0u;
        run += w;
        pre[i] = run;
    }
    unsigned long long total;
    const unsigned long long off = block_scan_u64(run, lds, total) - run;         // (its barrier orders n_pos = 0 in front of the adds)
#pragma unroll
    for (int i = 0; i < 4; ++i)
        if (n0 + i < N) wk.csum[n0 + i] = off + pre[i];
    if (pos) atomicAdd(&n_pos, pos);
    __syncthreads();
    if (threadIdx.x == 0) {
        wk.bsum[blockIdx.x] = total;
        if (n_pos) atomicAdd(&report[3], (unsigned long long)n_pos);
    }
}

// Weigh and scan: mcl_weigh_block, a block per MCL_SCAN_BLOCK particles
__global__ __launch_bounds__(MCL_SCAN_BLOCK / 4) void k_mcl_weigh(int N, const uint32_t* __restrict__ lut, int lut_n, int lut_shift, MclWork wk,
                                                                  unsigned long long* __restrict__ report) {
    mcl_weigh_block(N, lut, lut_n, lut_shift, wk, report);
}

// One block of MCL_SCAN_BLOCK threads: the scan blocks' sums become their exclusive prefix sums; W, the resampler's word and u0,
// and the report's words 0-15 that need no particle loop.  counted(t): thread t's share of word 5 -- the beams in range
// (mcl_beams_in_range) or the valid points (mclp_points_valid) among items t, t + MCL_SCAN_BLOCK, ...  KEEP15: word 15 is a sum the
// scoring launch has joined (the ray forms' through beams) and is left alone; every other form's word 15 is 0.
template <bool KEEP15 = false, class Counted>
__device__ __forceinline__ void mcl_sums_block(const int N, const uint64_t seed, const uint64_t scan, const Counted counted, const MclWork& wk,
                                               unsigned long long* __restrict__ report) {
    __shared__ unsigned long long lds[16];
    __shared__ unsigned n_rng;
    const int t = threadIdx.x, nb = (N + MCL_SCAN_BLOCK - 1) / MCL_SCAN_BLOCK;
    if (t == 0) n_rng = 0u;
    const unsigned long long v = t < nb ? wk.bsum[t] : 0ull;
    unsigned long long W;
    const unsigned long long incl = block_scan_u64(v, lds, W);
    if (t < nb) wk.bsum[t] = incl - v;
    const unsigned cnt = counted(t);
    if (cnt) atomicAdd(&n_rng, cnt);
    __syncthreads();
    if (t == 0) {
        const unsigned long long key = *wk.key, best = key & 0xfffffull;
        const unsigned long long r = philox4x32_10(0xffffffffu, 0u, (uint32_t)scan, (uint32_t)(scan >> 32), (uint32_t)seed, (uint32_t)(seed >> 32)).v[0];
        report[0] = key >> 20;
        report[1] = best;
        report[2] = W;
        report[4] = (W >> 32) * r + (((W & 0xffffffffull) * r) >> 32);          // floor(r * W / 2^32), W < 2^44
        report[5] = n_rng;
        for (int i = 0; i < 3; ++i) report[7 + i] = (unsigned long long)__double_as_longlong(wk.moved[best * 3 + i]);
        if (!KEEP15) report[15] = 0ull;
    }
}

// thread t's count of the scan's beams IN RANGE, for mcl_sums_block
__device__ __forceinline__ auto mcl_beams_in_range(const Slam2dLidar& lid, const double* __restrict__ ranges) {
    return [&lid, ranges](const int t) {
        unsigned cnt = 0u;
        for (int b = t; b < lid.beams; b += MCL_SCAN_BLOCK) cnt += ranges[b] < lid.max_range;
        return cnt;
    };
}

// Sums: mcl_sums_block, one block
__global__ __launch_bounds__(MCL_SCAN_BLOCK) void k_mcl_sums(Slam2dLidar lid, int N, uint64_t seed, uint64_t scan, const double* __restrict__ ranges,
                                                             MclWork wk, unsigned long long* __restrict__ report) {
    mcl_sums_block(N, seed, scan, mcl_beams_in_range(lid, ranges), wk, report);
}

// The resampler's pieces.  Offspring k of n_off has the ticket t_k = floor((k W + u0) / n_off) < W (below 2^64: W <= N * 0xffffff,
// N and n_off <= 2^20).
// The ancestor of ticket t among N particles: the least a with t < C_a, found in the scan blocks' prefix sums (block `start`s at
// bsum[lo]), then in that block's local ones (a = its i0-th particle).
struct MclAncestor { int a, i0; unsigned long long start; };
__device__ __forceinline__ MclAncestor mcl_ancestor(const unsigned long long t, const int N, const MclWork& wk) {
    const int nb = (N + MCL_SCAN_BLOCK - 1) / MCL_SCAN_BLOCK;
    int lo = 0, hi = nb - 1;                                                     // the least block whose inclusive end is beyond t
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (t < wk.bsum[mid + 1]) hi = mid; else lo = mid + 1;                   // (mid + 1 <= nb - 1: block mid's end is the next one's start)
    }
    const unsigned long long start = wk.bsum[lo], rel = t - start;
    const int base = lo * MCL_SCAN_BLOCK;
    int i0 = 0, i1 = min(MCL_SCAN_BLOCK, N - base) - 1;                          // rel < the block's sum = csum of its last particle
    while (i0 < i1) {
        const int mid = (i0 + i1) >> 1;
        if (rel < wk.csum[base + mid]) i1 = mid; else i0 = mid + 1;
    }
    return MclAncestor{base + i0, i0, start};
}
// k is its ancestor's FIRST offspring iff t_(k-1) falls in front of the ancestor's share -- the count of those is the number of
// distinct ancestors
__device__ __forceinline__ bool mcl_first_offspring(const int k, const MclAncestor& an, const unsigned long long W, const unsigned long long u0,
                                                    const int n_off, const MclWork& wk) {
    if (k <= 0) return true;                                                     // (offspring 0; k - 1 >= 0 below: an unsigned product)
    const unsigned long long tp = ((unsigned long long)(k - 1) * W + u0) / (unsigned long long)n_off;
    return tp < an.start + (an.i0 > 0 ? wk.csum[an.a - 1] : 0ull);
}
// Offspring k is particle a: the pose, the ancestor, and this thread's share of the report's sums into part[] -- first offspring,
// M, the four sums
__device__ __forceinline__ void mcl_emit_offspring(const int k, const int a, const bool first, const MclWork& wk, double* __restrict__ out,
                                                   const int pstride, int32_t* __restrict__ ancestor, unsigned long long (&part)[6]) {
    const double x = wk.moved[(size_t)a * 3], y = wk.moved[(size_t)a * 3 + 1], th = wk.moved[(size_t)a * 3 + 2];
    double* o = out + (size_t)k * pstride;
    o[0] = x; o[1] = y; o[2] = th;
    if (ancestor) ancestor[k] = a;
    part[0] += first;
    if (fabs(x) < 0x1p20 && fabs(y) < 0x1p20 && __builtin_isfinite(th)) {        // (a NaN fails the comparisons)
        part[1] += 1ull;
        part[2] += (unsigned long long)llrint(x * 65536.0);
        part[3] += (unsigned long long)llrint(y * 65536.0);
        part[4] += (unsigned long long)llrint(cos(th) * 0x1p30);
        part[5] += (unsigned long long)llrint(sin(th) * 0x1p30);
    }
}
// The threads' part[] joined per block in acc[] (zeroed in front of a barrier), then with integer atomics into the report's words
// 6 and 10-14.  Every thread of the block calls it.
__device__ __forceinline__ void mcl_join_sums(const unsigned long long (&part)[6], unsigned long long* acc, unsigned long long* __restrict__ report) {
#pragma unroll
    for (int i = 0; i < 6; ++i) {                                                // (every lane is here: signed sums in two's complement)
        const unsigned long long s = wave64_sum_u64(part[i]);
        if ((threadIdx.x & 63) == 0 && s) atomicAdd(&acc[i], s);
    }
    __syncthreads();
    if (threadIdx.x < 6 && acc[threadIdx.x]) atomicAdd(&report[threadIdx.x == 0 ? 6 : 9 + threadIdx.x], acc[threadIdx.x]);
}

// Resample: one thread per offspring k of N.  W == 0: every particle is its own offspring.
__global__ __launch_bounds__(256) void k_mcl_resample(int N, MclWork wk, double* __restrict__ out, int pstride, int32_t* __restrict__ ancestor,
                                                      unsigned long long* __restrict__ report) {
    __shared__ unsigned long long acc[6];
    if (threadIdx.x < 6) acc[threadIdx.x] = 0ull;
    __syncthreads();
    const int k = blockIdx.x * 256 + threadIdx.x;
    const unsigned long long W = report[2], u0 = report[4];
    unsigned long long part[6] = {0ull, 0ull, 0ull, 0ull, 0ull, 0ull};
    if (k < N) {
        int a = k;
        bool first = true;
        if (W) {
            const MclAncestor an = mcl_ancestor(((unsigned long long)k * W + u0) / (unsigned long long)N, N, wk);
            a = an.a;
            first = mcl_first_offspring(k, an, W, u0, N, wk);
        }
        mcl_emit_offspring(k, a, first, wk, out, pstride, ancestor, part);
    }
    mcl_join_sums(part, acc, report);
}

// ---- slam2d_mcl_step_adaptive: the same step over a LIVE count N that only the device knows, sized by the occupied pose bins ----
// No launch can be sized by N: every per-particle launch is a grid of at most MCLA_BLOCKS blocks (MCLA_SCORE_BLOCKS for the wave
// per particle of the scoring launch) that strides over n < N, so its cost follows N and not the capacity.  The loop bodies are
// the mcl_* bodies above, which the k_mcl_* kernels call too: one statement of each stage for both steps.
#define MCLA_BLOCKS 1024             // blocks of 256 threads: four per compute unit, 2^18 threads -- four particles each at 2^20
#define MCLA_SCORE_BLOCKS 2048       // blocks of MCL_WAVES waves: 32 waves per compute unit, a little more than its registers let it hold (28)
#define MCLA_REF_BLOCKS 512          // blocks of the reference-ancestor launch: fewer and longer, so that a block's filter sees more of a bin
#define MCLA_SEEN 1024               // entries of that filter: the bins a block has set already, direct-mapped in LDS
#define MCLA_TAIL 8                  // words of d_work behind the bitmap: |A|, kbins, then padding

__device__ __forceinline__ int mcla_live(const uint32_t* __restrict__ n_in, const int n_cap) {
    return (int)min(max(*n_in, 1u), (uint32_t)n_cap);
}
__host__ __device__ __forceinline__ long long mcla_bitmap_words(const long long n_bins) { return (n_bins + 64) / 64; }   // n_bins + 1 bits

// mcl_move_particle over n < N; thread 0 resets the joined words and the two counters of the tail, and the grid clears the bitmap
__global__ __launch_bounds__(256) void k_mcla_move(const uint32_t* __restrict__ n_in, int n_cap, const double* __restrict__ pose, int pstride,
                                                   double dfwd, double dside, double dturn, double amp0, double amp1, double amp2,
                                                   uint64_t seed, uint64_t scan, MclWork wk, unsigned long long* __restrict__ bitmap, int words,
                                                   unsigned long long* __restrict__ tail, unsigned long long* __restrict__ report) {
    const int N = mcla_live(n_in, n_cap), t0 = blockIdx.x * 256 + threadIdx.x, stride = gridDim.x * 256;
    if (t0 == 0) {
        mcl_reset_joined(wk, report);
        tail[0] = 0ull; tail[1] = 0ull;
    }
    for (int i = t0; i < words; i += stride) bitmap[i] = 0ull;
    for (int n = t0; n < N; n += stride) mcl_move_particle(n, pose, pstride, dfwd, dside, dturn, amp0, amp1, amp2, seed, scan, wk);
}

// mcl_score_particle: a wave takes particles wave, wave + the grid's waves, ... below N
__global__ __launch_bounds__(64 * MCL_WAVES) void k_mcla_score(Slam2dLidar lid, Slam2dLevel lv, int p_field, const uint32_t* __restrict__ n_in, int n_cap,
                                                               const double* __restrict__ ranges, unsigned outside_cost, MclWork wk) {
    const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int N = mcla_live(n_in, n_cap);
    const SlotField sf = slot_field(lv, p_field);
    for (int n = blockIdx.x * MCL_WAVES + wv; n < N; n += gridDim.x * MCL_WAVES)   // (wave-uniform)
        mcl_score_particle(n, lane, lid, lv, sf.fr, sf.fs, sf.field, ranges, outside_cost, wk);
}

// mcl_weigh_block, launched for the capacity: a block beyond N writes a zero sum and is done
__global__ __launch_bounds__(MCL_SCAN_BLOCK / 4) void k_mcla_weigh(const uint32_t* __restrict__ n_in, int n_cap, const uint32_t* __restrict__ lut, int lut_n,
                                                                   int lut_shift, MclWork wk, unsigned long long* __restrict__ report) {
    const int N = mcla_live(n_in, n_cap);
    if (blockIdx.x * MCL_SCAN_BLOCK >= N) {                                      // (block-uniform, in front of the first barrier)
        if (threadIdx.x == 0) wk.bsum[blockIdx.x] = 0ull;
        return;
    }
    mcl_weigh_block(N, lut, lut_n, lut_shift, wk, report);
}

// word 16 = N is what the last launch reads, as it may overwrite *n_in; the padding words
__device__ __forceinline__ void mcla_report_live(const int N, unsigned long long* __restrict__ report) {
    if (threadIdx.x == 0) {
        report[16] = (unsigned long long)N;
        for (int i = 20; i < 24; ++i) report[i] = 0ull;
    }
}

// mcl_sums_block, then mcla_report_live
__global__ __launch_bounds__(MCL_SCAN_BLOCK) void k_mcla_sums(Slam2dLidar lid, const uint32_t* __restrict__ n_in, int n_cap, uint64_t seed, uint64_t scan,
                                                              const double* __restrict__ ranges, MclWork wk, unsigned long long* __restrict__ report) {
    const int N = mcla_live(n_in, n_cap);
    mcl_sums_block(N, seed, scan, mcl_beams_in_range(lid, ranges), wk, report);
    mcla_report_live(N, report);
}

// The pose bin of the header's step e; n_bins for a pose that is not binnable.  No quotient that fails the guard is converted.
__device__ __forceinline__ int mcla_bin(const Slam2dMclBins& bn, const double x, const double y, const double th) {
    const double qx = (x - bn.x0) / bn.cell, qy = (y - bn.y0) / bn.cell, qt = th / bn.turn;
    const int n_bins = bn.nx * bn.ny * bn.nth;
    if (!(fabs(qx) < 1e9 && fabs(qy) < 1e9 && fabs(qt) < 1e9)) return n_bins;
    const int ix = (int)floor(qx), iy = (int)floor(qy);
    if (ix < 0 || ix >= bn.nx || iy < 0 || iy >= bn.ny) return n_bins;
    int it = (int)floor(qt) % bn.nth;
    if (it < 0) it += bn.nth;
    return (it * bn.ny + iy) * bn.nx + ix;
}

// Reference ancestors and their bins, a thread per particle and no search: n has an offspring among the N of the plain step iff
// the least k with k W + u0 >= C_(n-1) N is below N and has k W + u0 < C_n N (C N <= W N < 2^64; k W + u0 < N W).  Its bin's bit
// is set with an integer atomic OR, sent only where the word as last read lacks it -- and read only where the block's filter
// does not hold the bin: a set that has converged puts hundreds of thousands of members into a few dozen words, and without the
// filter every one of them goes to the same few L2 lines (profiles/r18_mcl_adaptive.md).  A filter entry is written by a thread
// that goes on to set that very bin, so a hit never loses a bit; a lost race costs an atomic.  |A| is counted per block, then
// atomically.
__global__ __launch_bounds__(256) void k_mcla_refs(const uint32_t* __restrict__ n_in, int n_cap, MclWork wk, Slam2dMclBins bn,
                                                   unsigned long long* __restrict__ bitmap, unsigned long long* __restrict__ tail,
                                                   const unsigned long long* __restrict__ report) {
    __shared__ unsigned n_ref;
    __shared__ int seen[MCLA_SEEN];
    if (threadIdx.x == 0) n_ref = 0u;
    for (int i = threadIdx.x; i < MCLA_SEEN; i += 256) seen[i] = -1;
    __syncthreads();
    const int N = mcla_live(n_in, n_cap);
    const unsigned long long W = report[2], u0 = report[4];
    unsigned long long cnt = 0ull;
    for (int n = blockIdx.x * 256 + threadIdx.x; n < N; n += gridDim.x * 256) {
        bool member = true;
        if (W) {
            const unsigned long long start = wk.bsum[n / MCL_SCAN_BLOCK];
            const unsigned long long lo = (start + (n % MCL_SCAN_BLOCK ? wk.csum[n - 1] : 0ull)) * (unsigned long long)N;
            const unsigned long long hi = (start + wk.csum[n]) * (unsigned long long)N;
            const unsigned long long k = lo > u0 ? (lo - u0 - 1ull) / W + 1ull : 0ull;      // ceil((lo - u0) / W)
            member = k < (unsigned long long)N && k * W + u0 < hi;
        }
        if (member) {
            const int bin = mcla_bin(bn, wk.moved[(size_t)n * 3], wk.moved[(size_t)n * 3 + 1], wk.moved[(size_t)n * 3 + 2]);
            int* slot = seen + (bin & (MCLA_SEEN - 1));
            if (*(volatile int*)slot != bin) {
                *(volatile int*)slot = bin;
                unsigned long long* word = bitmap + (bin >> 6);
                const unsigned long long bit = 1ull << (bin & 63);
                if (!(__hip_atomic_load(word, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) & bit)) atomicOr(word, bit);
            }
            ++cnt;
        }
    }
    cnt = wave64_sum_u64(cnt);                                                   // (every lane is here)
    if ((threadIdx.x & 63) == 0 && cnt) atomicAdd(&n_ref, (unsigned)cnt);
    __syncthreads();
    if (threadIdx.x == 0 && n_ref) atomicAdd(&tail[0], (unsigned long long)n_ref);
}

// kbins: the bitmap's population count
__global__ __launch_bounds__(256) void k_mcla_count(const unsigned long long* __restrict__ bitmap, int words, unsigned long long* __restrict__ tail) {
    __shared__ unsigned n_set;
    if (threadIdx.x == 0) n_set = 0u;
    __syncthreads();
    unsigned long long cnt = 0ull;
    for (int i = blockIdx.x * 256 + threadIdx.x; i < words; i += gridDim.x * 256) cnt += (unsigned long long)__popcll(bitmap[i]);
    cnt = wave64_sum_u64(cnt);
    if ((threadIdx.x & 63) == 0 && cnt) atomicAdd(&n_set, (unsigned)cnt);
    __syncthreads();
    if (threadIdx.x == 0 && n_set) atomicAdd(&tail[1], (unsigned long long)n_set);
}

// k_mcl_resample's pieces with N_out offspring of N particles: N from report word 16 (this launch writes *n_out, which may be
// *n_in), N_out from the table at kbins.  W == 0: a_j = j mod N, first offspring where j < N.
__global__ __launch_bounds__(256) void k_mcla_resample(int n_cap, const uint32_t* __restrict__ ntab, int ntab_n, MclWork wk,
                                                       const unsigned long long* __restrict__ tail, double* __restrict__ out, int pstride,
                                                       int32_t* __restrict__ ancestor, uint32_t* __restrict__ n_out,
                                                       unsigned long long* __restrict__ report) {
    __shared__ unsigned long long acc[6];
    if (threadIdx.x < 6) acc[threadIdx.x] = 0ull;
    __syncthreads();
    const int N = (int)report[16];
    const unsigned long long kbins = tail[1];
    const int N_out = (int)min(max(ntab[kbins < (unsigned long long)(ntab_n - 1) ? (int)kbins : ntab_n - 1], 1u), (uint32_t)n_cap);
    const unsigned long long W = report[2], u0 = report[4];
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        report[17] = (unsigned long long)N_out;
        report[18] = kbins;
        report[19] = tail[0];
        *n_out = (uint32_t)N_out;
    }
    unsigned long long part[6] = {0ull, 0ull, 0ull, 0ull, 0ull, 0ull};
    for (int j = blockIdx.x * 256 + threadIdx.x; j < N_out; j += gridDim.x * 256) {
        int a = j % N;
        bool first = j < N;
        if (W) {
            const MclAncestor an = mcl_ancestor(((unsigned long long)j * W + u0) / (unsigned long long)N_out, N, wk);
            a = an.a;
            first = mcl_first_offspring(j, an, W, u0, N_out, wk);
        }
        mcl_emit_offspring(j, a, first, wk, out, pstride, ancestor, part);
    }
    mcl_join_sums(part, acc, report);
}

// ---- the two steps with a charge per beam that crosses a wall (slam2d_mcl_step_rays, slam2d_mcl_step_adaptive_rays) ----
// WEIGH with slam2d_score_rays' THROUGH beams on a stride of the scan: the endpoint trips are mcl_beams, the ray pass behind them
// is ray_walk.  Only the move launch (it also resets word 15, which the scoring waves join), the score launch and the sums launch
// (it must not clear that word) differ from slam2d_mcl_step's: the weigh, reference, count and resample launches are its own.

// k_mcl_move, and word 15 = 0
__global__ __launch_bounds__(256) void k_mcl_move_rays(int N, const double* __restrict__ pose, int pstride, double dfwd, double dside, double dturn,
                                                       double amp0, double amp1, double amp2, uint64_t seed, uint64_t scan, MclWork wk,
                                                       unsigned long long* __restrict__ report) {
    const int n = blockIdx.x * 256 + threadIdx.x;
    if (n == 0) {
        mcl_reset_joined(wk, report);
        report[15] = 0ull;
    }
    if (n >= N) return;
    mcl_move_particle(n, pose, pstride, dfwd, dside, dturn, amp0, amp1, amp2, seed, scan, wk);
}

// k_mcla_move, and word 15 = 0
__global__ __launch_bounds__(256) void k_mcla_move_rays(const uint32_t* __restrict__ n_in, int n_cap, const double* __restrict__ pose, int pstride,
                                                        double dfwd, double dside, double dturn, double amp0, double amp1, double amp2,
                                                        uint64_t seed, uint64_t scan, MclWork wk, unsigned long long* __restrict__ bitmap, int words,
                                                        unsigned long long* __restrict__ tail, unsigned long long* __restrict__ report) {
    const int N = mcla_live(n_in, n_cap), t0 = blockIdx.x * 256 + threadIdx.x, stride = gridDim.x * 256;
    if (t0 == 0) {
        mcl_reset_joined(wk, report);
        report[15] = 0ull;
        tail[0] = 0ull; tail[1] = 0ull;
    }
    for (int i = t0; i < words; i += stride) bitmap[i] = 0ull;
    for (int n = t0; n < N; n += stride) mcl_move_particle(n, pose, pstride, dfwd, dside, dturn, amp0, amp1, amp2, seed, scan, wk);
}

#define MCLR_WAVES 16                // particles (waves) per block of the ray forms' scoring launches: one join of word 15 per block

// What the ray pass of a step takes beside the endpoint pass's arguments: the CAST beams (b % stride == phase), the margin and
// the charge, and where through_n goes (NULL: nowhere)
struct MclRays { int stride, phase, margin; unsigned through_cost; uint32_t* __restrict__ through; };

// Particle n on this wave: mcl_score_particle's endpoint trips -- mcl_beams, unchanged --, then the ray pass.  ray_walk is a
// wave-uniform loop that lasts as long as its longest ray, so a stride applied inside the endpoint trips would leave most lanes
// idle and still pay every trip; the CAST beams are packed over the lanes instead.  J = the number of cast beams; lane l of ray
// trip t takes cast beam j = 64 t + l, beam b = phase + j * stride (below B): 180 beams at stride 4 are 45 rays in ONE ray_walk.
// The lane evaluates its beam's a_b, cos and sin with the expression of the endpoint pass (fan.angle, cos, sin), so their bits are
// the endpoint's; CHECKED, kend and THROUGH are k_score_rays' lines.  Every ray ends: ray_walk's k strictly increases below
// k_exit <= kend + 1 < 2^30 (the quotient is below 1e9, margin >= 0), and a lane without a cast beam or with kend < 0 walks
// nothing.  through_n is joined by ballots; lane 0 writes the cost and d_through[n] and joins cost << 20 | n as mcl_score_particle
// does.  Returns through_n (the same on every lane) for mclr_join_block.
__device__ __forceinline__ int mcl_score_rays_particle(const int n, const int lane, const Slam2dLidar& lid, const Slam2dLevel& lv, const SlotField& sf,
                                                        const RayField& f, const double* __restrict__ ranges, const unsigned outside_cost,
                                                        const MclRays& ry, const MclWork& wk) {
    const double x = wk.moved[(size_t)n * 3], y = wk.moved[(size_t)n * 3 + 1], th = wk.moved[(size_t)n * 3 + 2];
    const int B = lid.beams, trips = (B + 63) >> 6;
    const BeamFan fan = fan_of(lid, th);
    unsigned long long sum_b = 0ull;                                             // (this lane's share)
    int n_in = 0, n_rng = 0, n_thr = 0;                                          // (the wave's counts: ballots)
    int t = 0;
    for (; t + MCL_UNROLL <= trips; t += MCL_UNROLL)                             // (wave-uniform trip counts)
        mcl_beams<MCL_UNROLL>(64 * t, lane, B, ranges, lid.max_range, fan, x, y, sf.fr, lv.step, sf.fs, lv.fpitch, sf.field, sum_b, n_in, n_rng);
    for (; t < trips; ++t) mcl_beams<1>(64 * t, lane, B, ranges, lid.max_range, fan, x, y, sf.fr, lv.step, sf.fs, lv.fpitch, sf.field, sum_b, n_in, n_rng);
    const int J = ry.phase < B ? (B - 1 - ry.phase) / ry.stride + 1 : 0;         // (phase + (J - 1) * stride <= B - 1)
    for (int j0 = 0; j0 < J; j0 += 64) {                                         // (wave-uniform trip count)
        const bool cast = j0 + lane < J;
        const int b = cast ? ry.phase + (j0 + lane) * ry.stride : 0;
        const double r = cast ? ranges[b] : NAN;
        const bool in_range = r < lid.max_range;                                 // (NaN and +inf are out, 0 and negatives in)
        const double a = fan.angle(b);
        const double q = r / f.step;
        const bool checked = in_range && q >= 0.0 && q < 1e9;
        const long long kend = checked ? (long long)q - ry.margin : -1ll;
        const uint32_t word = ray_walk(f, x, y, cos(a), sin(a), kend >= 0 ? (int)kend : 0, kend >= 0);
        const bool through = kend >= 0 && (word >> 30) == SLAM2D_RAY_HIT;           // (a HIT lies at k <= the limit, kend)
        n_thr += __popcll(__ballot(through));
    }
    sum_b = wave64_sum_u64(sum_b);
    if (lane == 0) {
        const unsigned long long cost = sum_b + (unsigned long long)(n_rng - n_in) * outside_cost
                                        + (unsigned long long)n_thr * ry.through_cost;                  // (below 2^44: two terms of at most 2^43)
        wk.cost[n] = cost;
        if (ry.through) ry.through[n] = (uint32_t)n_thr;
        const unsigned long long v = (cost << 20) | (unsigned long long)n;
        if (v < __hip_atomic_load(wk.key, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMin(wk.key, v);
    }
    return n_thr;
}

// The waves' through beams joined per block in LDS, then ONE integer atomic add on word 15, and none where the block has no
// through beam.  With an atomic per particle the waves of a large set send tens of thousands of them to the one address, and
// the launch waits for them, not for the rays: 0.52 ms of the 0.63 ms of a step of 65 536 particles at stride 4
// (profiles/r26_mcl_rays.md) -- what mclp_join_block met for the packed minimum.  Every thread of the block calls it.
__device__ __forceinline__ void mclr_join_block(const int thr, const int wv, const int lane, unsigned long long* __restrict__ report) {
    __shared__ int wthr[MCLR_WAVES];
    if (lane == 0) wthr[wv] = thr;
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned long long sum = 0ull;
        for (int i = 0; i < MCLR_WAVES; ++i) sum += (unsigned long long)wthr[i];
        if (sum) atomicAdd(&report[15], sum);
    }
}

// Score: one wave per particle (mcl_score_rays_particle), MCLR_WAVES of them per block (mclr_join_block).  Reads frames[p_field],
// the slot's field and squared distances, the moved poses and the ranges; writes the costs and d_through; no fault bit.
__global__ __launch_bounds__(64 * MCLR_WAVES) void k_mcl_score_rays(Slam2dLidar lid, Slam2dLevel lv, int p_field, const uint32_t* __restrict__ dist2, int N,
                                                                   const double* __restrict__ ranges, unsigned outside_cost, MclRays ry, MclWork wk,
                                                                   unsigned long long* __restrict__ report) {
    const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int n = blockIdx.x * MCLR_WAVES + wv;
    const SlotField sf = slot_field(lv, p_field);
    int thr = 0;
    if (n < N) thr = mcl_score_rays_particle(n, lane, lid, lv, sf, ray_field(lv, p_field, dist2), ranges, outside_cost, ry, wk);    // (wave-uniform)
    mclr_join_block(thr, wv, lane, report);
}

// mcl_score_rays_particle: a wave takes particles wave, wave + the grid's waves, ... below N and keeps their through beams for
// mclr_join_block
__global__ __launch_bounds__(64 * MCLR_WAVES) void k_mcla_score_rays(Slam2dLidar lid, Slam2dLevel lv, int p_field, const uint32_t* __restrict__ dist2,
                                                                    const uint32_t* __restrict__ n_in, int n_cap, const double* __restrict__ ranges,
                                                                    unsigned outside_cost, MclRays ry, MclWork wk,
                                                                    unsigned long long* __restrict__ report) {
    const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int N = mcla_live(n_in, n_cap);
    const SlotField sf = slot_field(lv, p_field);
    const RayField f = ray_field(lv, p_field, dist2);
    int thr = 0;                                                                 // (at most 2048 each of at most 2^20 particles: below 2^31)
    for (int n = blockIdx.x * MCLR_WAVES + wv; n < N; n += gridDim.x * MCLR_WAVES)  // (wave-uniform)
        thr += mcl_score_rays_particle(n, lane, lid, lv, sf, f, ranges, outside_cost, ry, wk);
    mclr_join_block(thr, wv, lane, report);
}

// k_mcl_sums and k_mcla_sums with word 15 kept
__global__ __launch_bounds__(MCL_SCAN_BLOCK) void k_mcl_sums_rays(Slam2dLidar lid, int N, uint64_t seed, uint64_t scan, const double* __restrict__ ranges,
                                                                  MclWork wk, unsigned long long* __restrict__ report) {
    mcl_sums_block<true>(N, seed, scan, mcl_beams_in_range(lid, ranges), wk, report);
}
__global__ __launch_bounds__(MCL_SCAN_BLOCK) void k_mcla_sums_rays(Slam2dLidar lid, const uint32_t* __restrict__ n_in, int n_cap, uint64_t seed,
                                                                   uint64_t scan, const double* __restrict__ ranges, MclWork wk,
                                                                   unsigned long long* __restrict__ report) {
    const int N = mcla_live(n_in, n_cap);
    mcl_sums_block<true>(N, seed, scan, mcl_beams_in_range(lid, ranges), wk, report);
    mcla_report_live(N, report);
}

// ---- the two steps for a set of points in the robot's frame (slam2d_mcl_step_points, slam2d_mcl_step_adaptive_points) ----
// WEIGH with the point cost of include/slam2d.h (above SLAM2D_MAX_POINTS): an endpoint is (x', y') + R(th') q.  A point's trip
// is six multiply-adds and two divisions, so one cos / sin per wave would cost more than the set's trips: the move launch, a
// thread per particle, evaluates cos(th'), sin(th') of the MOVED heading and leaves them in cs[n][2], 2 n words of d_work behind
// the scan form's, and the scoring wave evaluates no transcendental.  Only the move, score and sums launches differ from the
// scan forms': the weigh, reference, count and resample launches are theirs.

#define MCLP_WAVES 16                // particles (waves) per block of the point forms' scoring launches: one join per block

// mcl_move_particle, then the moved heading's cos / sin into cs
__device__ __forceinline__ void mclp_move_particle(const int n, const double* __restrict__ pose, const int pstride, const double dfwd, const double dside,
                                                   const double dturn, const double amp0, const double amp1, const double amp2, const uint64_t seed,
                                                   const uint64_t scan, const MclWork& wk, double* __restrict__ cs) {
    const double th = mcl_move_particle(n, pose, pstride, dfwd, dside, dturn, amp0, amp1, amp2, seed, scan, wk);
    cs[(size_t)n * 2] = cos(th);
    cs[(size_t)n * 2 + 1] = sin(th);
}

// k_mcl_move with mclp_move_particle
__global__ __launch_bounds__(256) void k_mclp_move(int N, const double* __restrict__ pose, int pstride, double dfwd, double dside, double dturn,
                                                   double amp0, double amp1, double amp2, uint64_t seed, uint64_t scan, MclWork wk,
                                                   double* __restrict__ cs, unsigned long long* __restrict__ report) {
    const int n = blockIdx.x * 256 + threadIdx.x;
    if (n == 0) mcl_reset_joined(wk, report);
    if (n >= N) return;
    mclp_move_particle(n, pose, pstride, dfwd, dside, dturn, amp0, amp1, amp2, seed, scan, wk, cs);
}

// mcl_beams for points: U trips of 64 points of one particle, from point k0.  A point that is not inside -- invalid, beyond the
// last point, outside the field, a quotient that fails the guard -- loads cell 0 of the image and adds nothing: no branch, so
// the U gathers are in flight together.  (An invalid point's offset is not finite, so its quotient fails the guard by itself.)
template <int U>
__device__ __forceinline__ void mclp_points(const int k0, const int lane, const int M, const double* __restrict__ pts, const int ptstride, const double c,
                                            const double s, const double x, const double y, const Slam2dFrame& fr, const double step,
                                            const FieldSize fs, const int fpitch, const uint32_t* __restrict__ field,
                                            unsigned long long& sum_b, int& n_in, int& n_val) {
    int idx[U];
    bool inside[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
        const int k = k0 + 64 * u + lane;
        const double qx = k < M ? pts[(size_t)k * ptstride] : NAN, qy = k < M ? pts[(size_t)k * ptstride + 1] : NAN;
        const bool valid = __builtin_isfinite(qx) && __builtin_isfinite(qy);     // (step 1)
        const double2 e = point_offset(c, s, qx, qy);
        int cx, cy;
        inside[u] = score_cell(x + e.x, y + e.y, fr.xlo, fr.ylo, step, fs.fw, fs.fh, cx, cy) && valid;
        idx[u] = inside[u] ? cy * fpitch + cx : 0;                               // (fmax * fpitch < 2^29)
        n_val += __popcll(__ballot(valid));
        n_in += __popcll(__ballot(inside[u]));
    }
    uint32_t cost[U];
#pragma unroll
    for (int u = 0; u < U; ++u) cost[u] = field[idx[u]];
#pragma unroll
    for (int u = 0; u < U; ++u) sum_b += inside[u] ? cost[u] : 0u;
}

// Particle n on this wave, as mcl_score_particle: the points interleaved over the lanes, read contiguously; the moved position and
// the heading's cos / sin from the move launch -- four doubles per particle.  Writes the particle's cost and returns cost << 20 | n
// (the same on every lane) for mclp_join_block.
__device__ __forceinline__ unsigned long long mclp_score_particle(const int n, const int lane, const Slam2dLevel& lv, const Slam2dFrame& fr, const FieldSize fs,
                                                    const uint32_t* __restrict__ field, const double* __restrict__ pts, const int ptstride, const int M,
                                                    const unsigned outside_cost, const MclWork& wk, const double* __restrict__ cs) {
    const double x = wk.moved[(size_t)n * 3], y = wk.moved[(size_t)n * 3 + 1], c = cs[(size_t)n * 2], s = cs[(size_t)n * 2 + 1];
    const int trips = (M + 63) >> 6;
    unsigned long long sum_b = 0ull;                                             // (this lane's share)
    int n_in = 0, n_val = 0;                                                     // (the wave's counts: ballots)
    int t = 0;
    for (; t + MCL_UNROLL <= trips; t += MCL_UNROLL)                             // (wave-uniform trip counts)
        mclp_points<MCL_UNROLL>(64 * t, lane, M, pts, ptstride, c, s, x, y, fr, lv.step, fs, lv.fpitch, field, sum_b, n_in, n_val);
    for (; t < trips; ++t) mclp_points<1>(64 * t, lane, M, pts, ptstride, c, s, x, y, fr, lv.step, fs, lv.fpitch, field, sum_b, n_in, n_val);
    sum_b = wave64_sum_u64(sum_b);
    const unsigned long long cost = sum_b + (unsigned long long)(n_val - n_in) * outside_cost;          // (below 2^44 at 2048 points)
    if (lane == 0) wk.cost[n] = cost;
    return (cost << 20) | (unsigned long long)n;
}

// The waves' minima of cost << 20 | n (all ones: none) joined per block in LDS, then with mcl_score_particle's conditional 64-bit
// atomicMin, one per block.  A wave of the point form is a few microseconds short: with a join per wave the waves of a small set
// all read the word before any atomic has landed and every one of them sends its own to the one address
// (profiles/r24_mcl_points.md).  Every thread of the block calls it.
__device__ __forceinline__ void mclp_join_block(const unsigned long long best, const int wv, const int lane, const MclWork& wk) {
    __shared__ unsigned long long wbest[MCLP_WAVES];
    if (lane == 0) wbest[wv] = best;
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned long long v = wbest[0];
        for (int i = 1; i < MCLP_WAVES; ++i) v = min(v, wbest[i]);
        if (v < __hip_atomic_load(wk.key, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMin(wk.key, v);
    }
}

// Score: one wave per particle (mclp_score_particle), MCLP_WAVES of them per block (mclp_join_block).  Reads frames[p_field], the
// slot's field, the moved poses, cs and the points; writes the costs; no fault bit.
__global__ __launch_bounds__(64 * MCLP_WAVES) void k_mclp_score(Slam2dLevel lv, int p_field, int N, const double* __restrict__ pts, int ptstride, int M,
                                                                unsigned outside_cost, MclWork wk, const double* __restrict__ cs) {
    const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int n = blockIdx.x * MCLP_WAVES + wv;
    const SlotField sf = slot_field(lv, p_field);
    unsigned long long best = ~0ull;
    if (n < N) best = mclp_score_particle(n, lane, lv, sf.fr, sf.fs, sf.field, pts, ptstride, M, outside_cost, wk, cs);    // (wave-uniform)
    mclp_join_block(best, wv, lane, wk);
}

// thread t's count of the set's VALID points, for mcl_sums_block
__device__ __forceinline__ auto mclp_points_valid(const double* __restrict__ pts, const int ptstride, const int M) {
    return [pts, ptstride, M](const int t) {
        unsigned cnt = 0u;
        for (int k = t; k < M; k += MCL_SCAN_BLOCK) cnt += point_valid(pts, ptstride, k);
        return cnt;
    };
}

// Sums: mcl_sums_block with the valid points in word 5, one block
__global__ __launch_bounds__(MCL_SCAN_BLOCK) void k_mclp_sums(int N, uint64_t seed, uint64_t scan, const double* __restrict__ pts, int ptstride, int M,
                                                              MclWork wk, unsigned long long* __restrict__ report) {
    mcl_sums_block(N, seed, scan, mclp_points_valid(pts, ptstride, M), wk, report);
}

// k_mcla_move with mclp_move_particle
__global__ __launch_bounds__(256) void k_mclap_move(const uint32_t* __restrict__ n_in, int n_cap, const double* __restrict__ pose, int pstride,
                                                    double dfwd, double dside, double dturn, double amp0, double amp1, double amp2,
                                                    uint64_t seed, uint64_t scan, MclWork wk, double* __restrict__ cs,
                                                    unsigned long long* __restrict__ bitmap, int words, unsigned long long* __restrict__ tail,
                                                    unsigned long long* __restrict__ report) {
    const int N = mcla_live(n_in, n_cap), t0 = blockIdx.x * 256 + threadIdx.x, stride = gridDim.x * 256;
    if (t0 == 0) {
        mcl_reset_joined(wk, report);
        tail[0] = 0ull; tail[1] = 0ull;
    }
    for (int i = t0; i < words; i += stride) bitmap[i] = 0ull;
    for (int n = t0; n < N; n += stride) mclp_move_particle(n, pose, pstride, dfwd, dside, dturn, amp0, amp1, amp2, seed, scan, wk, cs);
}

// mclp_score_particle: a wave takes particles wave, wave + the grid's waves, ... below N and keeps their minimum for mclp_join_block
__global__ __launch_bounds__(64 * MCLP_WAVES) void k_mclap_score(Slam2dLevel lv, int p_field, const uint32_t* __restrict__ n_in, int n_cap,
                                                                const double* __restrict__ pts, int ptstride, int M, unsigned outside_cost,
                                                                MclWork wk, const double* __restrict__ cs) {
    const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int N = mcla_live(n_in, n_cap);
    const SlotField sf = slot_field(lv, p_field);
    unsigned long long best = ~0ull;
    for (int n = blockIdx.x * MCLP_WAVES + wv; n < N; n += gridDim.x * MCLP_WAVES)  // (wave-uniform)
        best = min(best, mclp_score_particle(n, lane, lv, sf.fr, sf.fs, sf.field, pts, ptstride, M, outside_cost, wk, cs));
    mclp_join_block(best, wv, lane, wk);
}

// k_mclp_sums over the live count, then mcla_report_live
__global__ __launch_bounds__(MCL_SCAN_BLOCK) void k_mclap_sums(const uint32_t* __restrict__ n_in, int n_cap, uint64_t seed, uint64_t scan,
                                                               const double* __restrict__ pts, int ptstride, int M, MclWork wk,
                                                               unsigned long long* __restrict__ report) {
    const int N = mcla_live(n_in, n_cap);
    mcl_sums_block(N, seed, scan, mclp_points_valid(pts, ptstride, M), wk, report);
    mcla_report_live(N, report);
}

// Sharded normaliser, merge half: every rank folds the gathered [world][3] partials in rank order
// (so the result does not depend on the network's reduction order), normalises its own particles
// and evaluates sum (w - 1/N)^2 = sum w^2 - 1/N over ALL N particles (Algorithm/FastSlam.py:32-35).
__global__ __launch_bounds__(256) void k_weights_merge(double* logw, int N, const double* __restrict__ parts, int world,
                                                       double total_particles, double* w, double* stats,
                                                       const uint32_t* __restrict__ abort_flags, int abort_n, uint32_t abort_mask,
                                                       uint32_t* nsync = nullptr, const double* pack_d = nullptr, double* pack_h = nullptr,
                                                       int pack_n = 0, uint32_t* h_seq = nullptr, uint32_t seq = 0u) {
    if (abort_mask) {                                      // slam2d_groups_commit: a voided scan (see k_grid_update) has no partials to merge
        bool bad = false;
        for (int i = threadIdx.x; i < abort_n; i += blockDim.x) bad |= (abort_flags[i] & abort_mask) != 0u;
        if (__syncthreads_or(bad)) return;
    }
    bool voided = false;                                   // (a group of some rank left the VOID partial: k_grid_update's sharded abort)
    for (int r = 0; r < world; ++r) voided |= parts[3 * r + 1] < 0.0;
    double gm = -INFINITY;
    for (int r = 0; r < world; ++r) gm = fmax(gm, parts[3 * r]);
    double s1 = 0.0, s2 = 0.0;
    for (int r = 0; r < world; ++r) {
        const double sc = exp(parts[3 * r] - gm);
        s1 += parts[3 * r + 1] * sc;
        s2 += parts[3 * r + 2] * sc * sc;
    }
    const double lse = gm + log(s1);
    if (!voided)
        for (int i = threadIdx.x; i < N; i += 256) {
            const double lw = logw[i];
            w[i] = exp(lw - gm) / s1;
            logw[i] = lw - lse;
        }
    if (threadIdx.x == 0) {
        if (voided) { stats[0] = NAN; stats[1] = -1.0; }   // the report's marker: variance NaN, log of the sum -1 (a peer's NaN weights give NaN, NaN)
        else { stats[0] = s2 / (s1 * s1) - 1.0 / total_particles; stats[1] = lse; }
    }
    if (nsync && !voided) {                                // (slam2d_weights_merge_publish: the groups' next normaliser blocks wait for this)
        __syncthreads();
        if (threadIdx.x == 0) {
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
            const uint32_t gen = __hip_atomic_load(&nsync[1], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __hip_atomic_store(&nsync[1], gen + 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
    if (h_seq) {                                           // (slam2d_weights_merge_publish_report: the scan's pack to the host, as publish_pack)
        __syncthreads();
        for (int i = threadIdx.x; i < pack_n; i += blockDim.x) pack_h[i] = pack_d[i];
        __threadfence_system();
        __syncthreads();
        if (threadIdx.x == 0) __hip_atomic_store(h_seq, seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
    }
}

// The sharded normaliser without events between the groups and the normaliser's stream (round 5): the groups' blocks arrive on
// d_norm_sync[0] (normaliser_arrive), this one-wave kernel on the normaliser's stream waits for all of them -- they were enqueued
// before it -- and takes the counter back to zero; the all-gather of the partials and the merge follow on that stream, and the merge
// publishes d_norm_sync[1], which the groups' next normaliser blocks wait for (normaliser_wait).
__global__ __launch_bounds__(64) void k_norm_gate(uint32_t* nsync, int G) {
    if (threadIdx.x == 0) {
        const unsigned long long t0 = wall_clock64(), SYNC_SPIN_TICKS = sync_spin_ticks(nsync);
        bool late = false;
        while (__hip_atomic_load(&nsync[0], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < (uint32_t)G) {
            __builtin_amdgcn_s_sleep(8);
            if (wall_clock64() - t0 > SYNC_SPIN_TICKS) {           // (sticky: every later normaliser block raises the fault bit)
                __hip_atomic_store(&nsync[62], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                late = true;
                break;
            }
        }
        // (a tripped gate leaves the arrivals where they are: late groups still count themselves in, and the fault is fatal anyway)
        if (!late) __hip_atomic_store(&nsync[0], 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");          // (the partials: the collective behind this kernel reads them)
    }
}

// ------------------------------------------------------------------------------------
// K5  odometry prior / post-match bookkeeping          (Algorithm/FastSlam.py:77-120,131-135)
// ------------------------------------------------------------------------------------
__global__ void k_prior(const double* __restrict__ prev, double raw_theta, double prev_raw_theta, int has_turn,
                        double raw_turn, const double* __restrict__ heading, int P, double* est, double* psi_cs) {
    const int p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= P) return;
    prior_one(prev, heading, p, raw_theta, prev_raw_theta, has_turn, raw_turn, est, psi_cs);
}

// The closed loop's prior of a particle group with the scan's ranges PULLED from the caller's pinned host buffer in the same launch
// (Slam2dScan.h_ranges, ABI 16) into the group's own device buffer, which every later kernel of the group's scan reads -- instead
// of a copy-engine transfer and an event in front of every group's match.  (The uniforms, one per particle and read once by the
// selecting kernel, are read from the pinned buffer where they are used.)  Normally neither is launched: the previous scan's commit
// has written this scan's prior and pulled its ranges (Slam2dScan.h_next_ranges).
__global__ __launch_bounds__(256) void k_prior_pull(const double* __restrict__ prev, double raw_theta, double prev_raw_theta, int has_turn,
                                                    double raw_turn, const double* __restrict__ heading, int P, double* est, double* psi_cs,
                                                    const double* h_ranges, int B, double* d_pull) {
    for (int i = threadIdx.x; i < B; i += blockDim.x) d_pull[i] = __builtin_nontemporal_load(h_ranges + i);
    for (int p = threadIdx.x; p < P; p += blockDim.x) prior_one(prev, heading, p, raw_theta, prev_raw_theta, has_turn, raw_turn, est, psi_cs);
}
// Abort decision across groups without events (Slam2dScan.match_seq, ABI 16): the wave that writes a particle's result at the scan's
// LAST level counts the particle in (Slam2dLevel.arrive = word 61 of the sync block: particle-matches finished since the words were
// zeroed); every group's commit starts with k_abort_gate, ONE wave that waits -- bounded -- until all particles of all groups of this
// scan's match call have been counted: the update launch behind it then reads every group's fault bits as it did behind the events.
// No deadlock, whatever hardware queues the groups' streams share: a commit call is issued after the match call of ALL groups has
// been issued completely, so everything a gate waits for sits in front of it in every queue; and only one wave per group waits.
// (A gate that counted its own group in -- one launch less per match -- deadlocked with eight groups on eight hardware queues, one
// of them the default stream's: two groups shared a queue and the first gate waited for the one queued behind it.)
__global__ __launch_bounds__(64) void k_abort_gate(uint32_t* nsync, uint32_t want, uint32_t* flags) {
    if (threadIdx.x == 0) {
        const unsigned long long t0 = wall_clock64(), SYNC_SPIN_TICKS = sync_spin_ticks(nsync);
        while ((int)(__hip_atomic_load(&nsync[61], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) - want) < 0) {
            __builtin_amdgcn_s_sleep(8);
            if (wall_clock64() - t0 > SYNC_SPIN_TICKS) { atomicOr(&flags[0], SLAM2D_F_SYNC_TIMEOUT); break; }
        }
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
    }
}
__global__ __launch_bounds__(64) void k_match_arrive(uint32_t* nsync, uint32_t n) {       // (single-level matches: no level to carry the word)
    if (threadIdx.x == 0) __hip_atomic_fetch_add(&nsync[61], n, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__global__ void k_post_match(const Slam2dMatch* __restrict__ fine, const Slam2dMatch* __restrict__ coarse, int P,
                             double* prev, double* heading, double* logw, double* report) {
    const int p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p < P) post_match_one(fine, coarse, p, prev, heading, logw, report);
}

// ------------------------------------------------------------------------------------
// resample state movement / fill
// ------------------------------------------------------------------------------------
__global__ void k_gather_maps(const Slam2dMap* __restrict__ src, const Slam2dMap* __restrict__ dst,
                              const int32_t* __restrict__ index) {
    const int p = blockIdx.y;
    const Slam2dMap s = src[index[p]], d = dst[p];
    const size_t n = (size_t)s.rows * s.pitch * (s.wide ? 2 : 1);          // 32-bit words (a wide map: two per cell)
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x)
        d.cells[i] = s.cells[i];
}

// The picture of a map the reference draws (Algorithm/FastSlam.py:172-176): 1 - visited / total over a window, optionally
// flipped upside down (np.flipud); float64 like the reference's arrays and / or 8-bit grey.
__global__ void k_map_image(const Slam2dMap* __restrict__ maps, int p, int x0, int y0, int w, int h, int flipud,
                            double* out, uint8_t* out_u8) {
    const Slam2dMap m = maps[p];
    const long long n = (long long)w * h;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
        const int r = (int)(i / w), c = (int)(i - (long long)r * w);
        const int my = flipud ? y0 + (h - 1 - r) : y0 + r;
        double vis, tot;
        if (m.wide) {
            const unsigned long long v = reinterpret_cast<const unsigned long long*>(m.cells)[(size_t)my * m.pitch + x0 + c];
            vis = (double)(v >> 32); tot = (double)(v & 0xffffffffull);
        } else {
            const uint32_t v = m.cells[(size_t)my * m.pitch + x0 + c];
            vis = (double)(v >> 16); tot = (double)(v & 0xffffu);
        }
        const double val = 1.0 - vis / tot;                                     // ogMap = visited / total; 1 - ogMap (:173,176)
        if (out) out[i] = val;
        if (out_u8) out_u8[i] = (uint8_t)rint(fmin(fmax(val, 0.0), 1.0) * 255.0);
    }
}

__global__ void k_fill(uint32_t* cells, long long n, uint32_t value) {
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x)
        cells[i] = value;
}

// ------------------------------------------------------------------------------------
// Pose mean and covariance of a match (slam2d_match_moments): every pose of the cube is scored again through the
// exact-score core k_sweep scores it with -- Acc4 over the unique endpoint cells, pose_score with the two prior planes -- and turned
// into the weight w = exp(score - M), M = Slam2dMatch.best_score; the cube itself is neither read nor written (after branch and
// bound it holds only the scored tiles, and the skipped poses' mass times offset^2 is not negligible for a second moment).
// k_sweep's work shape: a block per (particle, theta, chunk of 64 slots), a lane owns the 4 consecutive dx of one slot through
// one 16-byte buffer load per cell, the block's four waves split the cell list and meet in LDS.  Wave 0 then reduces
// w, w * d, w * d d^T (d = offset from the ARG-MAX pose in metres / radians: the moments are shifted to the mean at the end,
// where E[d d^T] - E[d] E[d]^T then subtracts numbers of the covariance's own size) with wave_sum -- a fixed order -- and leaves
// one row of MOMENTS_ROW doubles per block in d_work.  k_moments_fold, one wave per particle, adds a particle's rows in index
// order (a lane takes a contiguous run of rows, the lanes meet in wave_sum) and writes the SLAM2D_MOMENTS_STRIDE output doubles.
// No atomics: the same inputs give the same bits on every call.
// ------------------------------------------------------------------------------------
#define MOMENTS_ROW 12               // sum w | sum w d (x, y, theta) | sum w d d^T (xx, xy, xt, yy, yt, tt) | poses | NaN scores
__device__ __forceinline__ int moments_argmax(const Slam2dLevel& lv, const Slam2dMatch* __restrict__ match, const int p) {
    const int a = match[p].argmax;
    return (a >= 0 && a < lv.ntheta * cube_of(lv).npose) ? a : 0;         // (a record nobody wrote: any pose serves as the origin)
}
__global__ __launch_bounds__(256) void k_moments(Slam2dLevel lv, int P, int chunks, int bpp, const Slam2dMatch* __restrict__ match,
                                                 double* __restrict__ work) {
    __shared__ unsigned long long part_s[3][WAVE * 4];
    int p, w;
    xcd_particle(blockIdx.x, bpp, &p, &w);
    if (p >= P) return;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    const int it = w / chunks, ch = w - it * chunks;
    const Cube cube = cube_of(lv);
    const int nx = cube.nx, npose = cube.npose;
    const int* __restrict__ cl = lv.cells + ((size_t)p * lv.ntheta + it) * lv.kmax;
    const int K = min(lv.kcount[p * lv.ntheta + it], lv.kmax);
    const __amdgpu_buffer_rsrc_t rsrc = field_rsrc(lv, p);
    const Slot sl = slot_of(cube, lv.fpitch, ch * WAVE + lane);   // the lane's slot
    const int iy = sl.iy, dx = sl.dx, off = sl.off, nv = sl.nv;
    Acc4 sum4;
#pragma unroll 4
    for (int k = wave; k < K; k += 4) {
        const int cell = cl[k] * 4;
        sum4.add(__builtin_amdgcn_raw_buffer_load_b128(rsrc, off, cell, 0));
    }
    if (wave > 0) {
#pragma unroll
        for (int e = 0; e < 4; ++e) part_s[wave - 1][e * WAVE + lane] = sum4.get(e);
    }
    __syncthreads();
    if (wave > 0) return;
    const double inv = 1.0 / lv.cost_scale;
    const double M = match[p].best_score;
    const int am = moments_argmax(lv, match, p);
    const int ita = am / npose, rema = am - ita * npose;
    const int iya = rema / nx, ixa = rema - iya * nx;
    const double dth = lv.thetas[it] - lv.thetas[ita];
    const double dyv = (double)(iy - iya) * lv.step;
    double prv[4], ptw[4];
    slot_priors(lv.prior + (size_t)p * 2 * npose, cube, sl.q0, prv, ptw);
    double s0 = 0.0, sx = 0.0, sy = 0.0, st = 0.0, sxx = 0.0, sxy = 0.0, sxt = 0.0, syy = 0.0, syt = 0.0, stt = 0.0;
    double cnt = 0.0, cnan = 0.0;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        if (e < nv) {
            const unsigned long long acc = sum4.get(e) + part_s[0][e * WAVE + lane] + part_s[1][e * WAVE + lane] + part_s[2][e * WAVE + lane];
            const double sc = pose_score(acc, inv, prv[e], ptw[e]);
            const double wgt = exp(sc - M);
            const double dxv = (double)(dx + e - ixa) * lv.step;
            s0 += wgt;
            sx += wgt * dxv; sy += wgt * dyv; st += wgt * dth;
            sxx += wgt * (dxv * dxv); sxy += wgt * (dxv * dyv); sxt += wgt * (dxv * dth);
            syy += wgt * (dyv * dyv); syt += wgt * (dyv * dth); stt += wgt * (dth * dth);
            cnt += 1.0;
            cnan += isnan(sc) ? 1.0 : 0.0;
        }
    }
    double row[MOMENTS_ROW] = {s0, sx, sy, st, sxx, sxy, sxt, syy, syt, stt, cnt, cnan};
#pragma unroll
    for (int i = 0; i < MOMENTS_ROW; ++i) row[i] = wave_sum(row[i]);
    if (lane == 0) {
        double* dst = work + (((size_t)p * lv.ntheta + it) * chunks + ch) * MOMENTS_ROW;
#pragma unroll
        for (int i = 0; i < MOMENTS_ROW; ++i) dst[i] = row[i];
    }
}

__global__ __launch_bounds__(64) void k_moments_fold(Slam2dLevel lv, int nrows, const Slam2dMatch* __restrict__ match,
                                                     const double* __restrict__ work, double* __restrict__ out) {
    const int p = blockIdx.x, lane = threadIdx.x;
    const double* __restrict__ rows = work + (size_t)p * nrows * MOMENTS_ROW;
    const int per = (nrows + WAVE - 1) / WAVE;
    const int r0 = min(nrows, lane * per), r1 = min(nrows, r0 + per);
    double acc[MOMENTS_ROW];
#pragma unroll
    for (int i = 0; i < MOMENTS_ROW; ++i) acc[i] = 0.0;
    for (int r = r0; r < r1; ++r)
#pragma unroll
        for (int i = 0; i < MOMENTS_ROW; ++i) acc[i] += rows[(size_t)r * MOMENTS_ROW + i];
#pragma unroll
    for (int i = 0; i < MOMENTS_ROW; ++i) acc[i] = wave_sum(acc[i]);
    if (lane != 0) return;
    const int nx = cube_of(lv).nx, npose = cube_of(lv).npose;
    const int am = moments_argmax(lv, match, p);
    const int ita = am / npose, rema = am - ita * npose;
    const int iya = rema / nx, ixa = rema - iya * nx;
    double* o = out + (size_t)p * SLAM2D_MOMENTS_STRIDE;
    const double s0 = acc[0];
    const double mx = acc[1] / s0, my = acc[2] / s0, mt = acc[3] / s0;              // mean offset from the arg-max pose
    o[0] = s0;
    o[1] = (double)(ixa - lv.ncell) * lv.step + mx;                                // ... from the estimate
    o[2] = (double)(iya - lv.ncell) * lv.step + my;
    o[3] = lv.thetas[ita] + mt;
    o[4] = acc[4] / s0 - mx * mx; o[5] = acc[5] / s0 - mx * my; o[6] = acc[6] / s0 - mx * mt;
    o[7] = acc[7] / s0 - my * my; o[8] = acc[8] / s0 - my * mt; o[9] = acc[9] / s0 - mt * mt;
    if (acc[11] > 0.0)                                                             // a NaN score: exp(NaN) made them NaN already
        for (int i = 0; i < 10; ++i) o[i] = NAN;
    o[10] = match[p].best_score;
    o[11] = acc[10];
    o[12] = acc[11];
    o[13] = 0.0; o[14] = 0.0; o[15] = 0.0;
}

// ------------------------------------------------------------------------------------
// C ABI
// ------------------------------------------------------------------------------------
// slots of 4 consecutive dx in a plane of the level's cube, and the chunks of 64 slots (one per lane) k_sweep and k_moments cut it into
static int cube_slots(const Slam2dLevel& lv) { return cube_of(lv).nslot; }
static int cube_chunks(const Slam2dLevel& lv) { return cdiv(cube_slots(lv), WAVE); }

static void launch_sweep(const Slam2dLevel& lv, int P, int chunks, hipStream_t s, int mode = 0, const double* sel_est = nullptr,
                         int sel_estride = 0, Slam2dMatch* sel_out = nullptr) {
    const int bpp = lv.ntheta * cdiv(chunks, mode == 2 ? SWEEP_REST_CHUNKS : (mode == 0 ? SWEEP_MAIN_CHUNKS : 1));   // blocks per particle
    const unsigned grid = cdiv(P, 8) * 8 * bpp;
    if (mode == 1) { k_sweep<1, false><<<grid, 256, 0, s>>>(lv, P, chunks, bpp); return; }
    // worth it for long cell lists (measured: 1081 beams -15 %, 180 beams +4 %: the vector prologue of the skip
    // loop costs more than 29 % fewer loads save when a wave has only ~43 cells)
    if (sweep_skips(lv)) {
        if (mode == 0) k_sweep<0, true><<<grid, 256, 0, s>>>(lv, P, chunks, bpp, sel_est, sel_estride, sel_out);
        else k_sweep<2, true><<<grid, 256, 0, s>>>(lv, P, chunks, bpp);
        return;
    }
    // deep: SWEEP_DEPTH gathers in flight per wave, where the launch is about one round of blocks
    const int deep = bpp <= SWEEP_DEEP_MAX_BLOCKS ? 1 : 0;
    if (mode == 0) k_sweep<0, false><<<grid, 256, 0, s>>>(lv, P, chunks, bpp, sel_est, sel_estride, sel_out, deep);
    else k_sweep<2, false><<<grid, 256, 0, s>>>(lv, P, chunks, bpp, nullptr, 0, nullptr, deep);
}

// More dynamic LDS than the default limit for `kernel`: asked for once per device (`granted`: the kernel's own record; 160 KB
// per CU on gfx950).  false: more than a CU has, or the device does not grant it -- the caller reports a clean error or falls
// back instead of a failed launch.
constexpr size_t DYN_LDS_MAX = 160 * 1024 - 512;
static bool grant_dynamic_lds(const void* kernel, size_t (&granted)[64], size_t lds) {
    int dev = 0;
    (void)hipGetDevice(&dev);
    size_t& allowed = granted[dev >= 0 && dev < 64 ? dev : 0];
    if (allowed == 0) allowed = 64 * 1024;
    if (lds <= allowed) return true;
    if (lds > DYN_LDS_MAX || hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)DYN_LDS_MAX) != hipSuccess) {
        (void)hipGetLastError();
        return false;
    }
    allowed = DYN_LDS_MAX;
    return true;
}
// How k_bound_lds runs at a level (bound_lds_plan): ok = it does -- every condition of its launch, the dynamic-LDS grant included,
// was evaluated when the plan was made, so whoever reads the plan (the field build's fold, the launch) sees one decision.
struct BoundLdsPlan { bool ok; int nset; bool rle; int bpp, tpb, nw; size_t lds; bool hoist; };      // hoist: the form with a list-head slot per wave
// one instantiation of k_bound_lds: its LDS granted (launch == false: that is all; false: not granted), then launched
template <int NSET, bool RLE, bool HOIST = false>
static bool bound_lds_as(const Slam2dLevel& lv, int P, const BoundLdsPlan& pl, bool launch, int refresh, hipStream_t s) {
    static size_t granted[64] = {};
    if (!grant_dynamic_lds(reinterpret_cast<const void*>(k_bound_lds<NSET, RLE, HOIST>), granted, pl.lds)) return false;
    if (launch) k_bound_lds<NSET, RLE, HOIST><<<(unsigned)cdiv(P, 8) * 8 * pl.bpp, WAVE * pl.nw, pl.lds, s>>>(lv, P, pl.bpp, pl.tpb, refresh);
    return true;
}
static bool bound_lds_dispatch(const Slam2dLevel& lv, int P, const BoundLdsPlan& pl, bool launch, int refresh, hipStream_t s) {
    switch ((pl.nset - 1) * 2 + (pl.rle ? 1 : 0)) {
        case 0: return pl.hoist ? bound_lds_as<1, false, true>(lv, P, pl, launch, refresh, s) : bound_lds_as<1, false>(lv, P, pl, launch, refresh, s);
        case 1: return bound_lds_as<1, true>(lv, P, pl, launch, refresh, s);
        case 2: return pl.hoist ? bound_lds_as<2, false, true>(lv, P, pl, launch, refresh, s) : bound_lds_as<2, false>(lv, P, pl, launch, refresh, s);
        case 3: return bound_lds_as<2, true>(lv, P, pl, launch, refresh, s);
        case 4: return bound_lds_as<3, false>(lv, P, pl, launch, refresh, s);
        case 5: return bound_lds_as<3, true>(lv, P, pl, launch, refresh, s);
        case 6: return bound_lds_as<4, false>(lv, P, pl, launch, refresh, s);
        default: return bound_lds_as<4, true>(lv, P, pl, launch, refresh, s);
    }
}

extern "C" {

int slam2d_abi_version(void) { return SLAM2D_ABI_VERSION; }

int slam2d_sizeof(const char* name) {
    if (!name) return -1;
    if (!strcmp(name, "Slam2dMap")) return (int)sizeof(Slam2dMap);
    if (!strcmp(name, "Slam2dLidar")) return (int)sizeof(Slam2dLidar);
    if (!strcmp(name, "Slam2dFrame")) return (int)sizeof(Slam2dFrame);
    if (!strcmp(name, "Slam2dLevel")) return (int)sizeof(Slam2dLevel);
    if (!strcmp(name, "Slam2dMatch")) return (int)sizeof(Slam2dMatch);
    if (!strcmp(name, "Slam2dPartial")) return (int)sizeof(Slam2dPartial);
    if (!strcmp(name, "Slam2dGroup")) return (int)sizeof(Slam2dGroup);
    if (!strcmp(name, "Slam2dScan")) return (int)sizeof(Slam2dScan);
    if (!strcmp(name, "Slam2dBeamPlan")) return (int)sizeof(Slam2dBeamPlan);
    if (!strcmp(name, "Slam2dMclBins")) return (int)sizeof(Slam2dMclBins);
    return -1;
}

int slam2d_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) { (void)hipGetLastError(); return 0; }
    return n;
}

static int check_level(const Slam2dLidar* lidar, const Slam2dLevel* lv, int P) {
    if (!lidar || !lv || P <= 0) return SLAM2D_E_BADARG;
    if (lv->blur_radius < 0 || lv->blur_radius > SLAM2D_MAX_BLUR_RADIUS) return SLAM2D_E_TOOLARGE;
    if (lidar->beams < 2 || lidar->beams > SLAM2D_MAX_BEAMS) return SLAM2D_E_TOOLARGE;
    if (lv->fmax <= 0 || lv->fpitch < lv->fmax || lv->wmax <= 0 || lv->ncell < 0 || lv->ntheta <= 0) return SLAM2D_E_BADARG;
    if (!(lv->cost_scale > 0.0)) return SLAM2D_E_BADARG;
    if ((long long)lv->fmax * lv->fpitch >= (1ll << 29)) return SLAM2D_E_TOOLARGE;     // byte offsets into one field stay below 2^31
    return 0;
}

// ---- launch sequences shared by slam2d_field_build / slam2d_sweep / slam2d_match ----
static int check_field_args(const Slam2dLevel& lv, int P, bool lazy) {
    // (occ and tilemask are cleared by ONE memset when occ_gen == 0; with generation stamps nothing is cleared and a level may
    // be an offset view of a larger one -- slam2d_groups_* -- whose flags do not follow its image)
    if (!lv.occ || !lv.tilemask || (lv.occ_gen == 0 && lv.tilemask != lv.occ + (size_t)P * lv.fmax * lv.fpitch) || !lv.tilestate || !lv.tilemin || !lv.tilemax || !lv.tilelist || !lv.tilecount)
        return SLAM2D_E_BADARG;
    if (lazy && !lv.tileneed) return SLAM2D_E_BADARG;
    if (lv.tmax * lv.tmax > 28000) return SLAM2D_E_TOOLARGE;        // k_tile_triage: 32 passes, 5 bytes of LDS per tile (144 KB)
    const Cube cube = cube_of(lv);
    const int nx = cube.nx;
    if (lv.bnb == 3) {                                 // angle bounds: small cubes only, windows of <= 5 x 5 cells
        if (!lazy || !lv.gmin || !lv.gmin2 || !lv.pcells || !lv.bounds || !lv.bnb_best || !lv.seed_key) return SLAM2D_E_BADARG;
        if (nx > 5 || cube.nslot > 32 || lv.tmax * 16 != lv.fpitch || lv.ntheta >= (1 << 14)) return SLAM2D_E_BADARG;
    } else if (lv.bnb) {
        if (!lazy || !lv.gmin || !lv.gmin2 || !lv.pcells || !lv.bounds || !lv.tile_pmax || !lv.bnb_best || !lv.prune_state)
            return SLAM2D_E_BADARG;
        if (lv.bnb == 2 && (!lv.gmin3d || !lv.p3cells || !lv.bounds1 || !lv.seed_key || (lv.tmax & 0) != 0)) return SLAM2D_E_BADARG;
        if (nx < 9 || nx > 64 || lv.tmax * 16 != lv.fpitch) return SLAM2D_E_BADARG;
        if (lv.ntheta > SLAM2D_BNB_MAX_THETA) return SLAM2D_E_TOOLARGE;
        if ((long long)lv.ntheta * cube.nbt * cube.nbq4 > (long long)XS_THREADS * XS_MAX_PER) return SLAM2D_E_TOOLARGE;
    }
    return 0;
}

// frame geometry, axis index vectors, cleared occupancy image / tile flags (/ needed-tile bitmap)
static int launch_frames(const Slam2dLidar& lid, const Slam2dLevel& lv, const Slam2dMap* d_maps, int P,
                         const double* d_centre, int centre_stride, uint32_t* d_flags, bool lazy, hipStream_t s,
                         const double* d_ranges = nullptr) {
    if (d_ranges && (!lv.beam_xy || centre_stride < 3)) d_ranges = nullptr;
    k_frame_axis<<<dim3(cdiv(lv.wmax, 256), P, 2), 256, 0, s>>>(lid, lv, d_maps, d_centre, centre_stride, d_flags, d_ranges);
    if (lv.occ_gen < 0 || lv.occ_gen > 255) return SLAM2D_E_BADARG;
    if (lv.occ_gen != 0) return 0;                     // generation stamps: nothing to clear
    return (int)hipMemsetAsync(lv.occ, 0, (size_t)P * lv.fmax * lv.fpitch + (size_t)P * flag_bytes(lv), s);
}

// occupied cells -> field image, tile triage (+ fill), blur + clamp, minimum check
// Is k_blur_check_redo's launch folded away at this level?  Without the sweep's free-tile masks and without the prior pruning
// (which reads the field's maximum) it has two duties left.  The minimum check of a frame without a free tile: the blur's last
// block does it (k_blur_clamp, tail; its arrival counter is lv.sync word 1 -- k_exact_select counts in word 0, the sweep's fused
// selection in word 2).  The bound minima gmin2 / gmin2b of the tiles just written: without bounds there are none (round 4: one
// launch per level less, 2 x 6 us per scan at the reference's defaults); with bounds taken by k_bound_lds (bound_lds: the
// level's BoundLdsPlan.ok) that kernel's prologue derives them.  Two-level and angle bounds, the full build and k_bound keep the launch.
static bool fold_field_check(const Slam2dLevel& lv, bool lazy, bool field_max_needed, bool bound_lds) {
    return lazy && (lv.bnb == 0 || (lv.bnb == 1 && bound_lds)) && !sweep_skips(lv) && !field_max_needed && lv.sync != nullptr;
}
static void launch_scatter(const Slam2dLevel& lv, const Slam2dMap* d_maps, int P, hipStream_t s) {
    StageScope prof(SLAM2D_STAGE_SCATTER, s);
    k_occ_scatter<<<dim3(cdiv(cdiv(lv.wmax, 32) + 1, 64), cdiv(lv.wmax, SCATTER_ROWS), P), dim3(64, 4), (size_t)lv.wmax * sizeof(int32_t), s>>>(lv, d_maps);
}
static int launch_field(const Slam2dLevel& lv, const Slam2dMap* d_maps, int P, uint32_t* d_flags, bool lazy, hipStream_t s,
                        bool scattered = false, bool field_max_needed = true, bool bound_lds = false) {
    if (!scattered) launch_scatter(lv, d_maps, P, s);
    const int ntile = lv.tmax * lv.tmax;
    const bool folded = fold_field_check(lv, lazy, field_max_needed, bound_lds);
    {
        const int kb = (lv.blur_radius + 7) >> FLAG_SHIFT;
        const int rw = (flag_pitch(lv) >> 4) + 1;
        const size_t lds = (size_t)((2 * ((((2 * lv.tmax + 2 * kb) * rw + 1) & ~1) + lv.tmax * (rw + 1)) + 15) & ~15) + ((ntile + 3) & ~3) + 4 * ((ntile + 31) / 32) + 2 * (size_t)ntile;
        static size_t granted[64] = {};
        if (!grant_dynamic_lds(reinterpret_cast<const void*>(k_tile_triage), granted, lds)) return SLAM2D_E_TOOLARGE;
        k_tile_triage<<<P, TRIAGE_THREADS, lds, s>>>(lv, lazy ? 1 : 0);
    }
    {
        StageScope prof(SLAM2D_STAGE_BLUR, s);
        const int bpp = min(ntile, SLAM2D_BLUR_BLOCKS_PER_PARTICLE);
        const unsigned bgrid = (unsigned)cdiv(P, 8) * 8 * bpp;
        const int tail = folded ? 1 : 0;
        switch (lv.blur_radius) {
            case 2: k_blur_clamp<2><<<bgrid, BLUR_THREADS, 0, s>>>(lv, P, bpp, d_flags, tail); break;
            case 4: k_blur_clamp<4><<<bgrid, BLUR_THREADS, 0, s>>>(lv, P, bpp, d_flags, tail); break;
            case 8: k_blur_clamp<8><<<bgrid, BLUR_THREADS, 0, s>>>(lv, P, bpp, d_flags, tail); break;
            default: k_blur_clamp<0><<<bgrid, BLUR_THREADS, 0, s>>>(lv, P, bpp, d_flags, tail); break;
        }
    }
    if (folded) return 0;                              // the minimum check rode in the blur's launch: nothing else to do at this level
    const int dirty = lazy ? 1 : 0;                    // gmin2 only where a tile was written (the full build: over the whole frame)
    const dim3 cgrid(P, lv.bnb ? GMIN2_BLOCKS : 1);
    switch (lv.blur_radius) {
        case 2: k_blur_check_redo<2><<<cgrid, 256, 0, s>>>(lv, d_flags, dirty); break;
        case 4: k_blur_check_redo<4><<<cgrid, 256, 0, s>>>(lv, d_flags, dirty); break;
        case 8: k_blur_check_redo<8><<<cgrid, 256, 0, s>>>(lv, d_flags, dirty); break;
        default: k_blur_check_redo<0><<<cgrid, 256, 0, s>>>(lv, d_flags, dirty); break;
    }
    return 0;
}

// beam endpoints, unique cells per theta, priors (/ needed tiles)
static void launch_endpoints(const Slam2dLidar& lid, const Slam2dLevel& lv, int P, const double* d_est, int est_stride,
                             const double* d_ranges, double est_moving_dist, const double* d_psi_cs, uint32_t* d_flags,
                             bool mark, bool prune, hipStream_t s, bool beam_table = false,
                             const Slam2dMap* own_frame_maps = nullptr) {
    StageScope prof(SLAM2D_STAGE_ENDPOINTS, s);
    int n = 256;
    while (n < lid.beams) n <<= 1;
    const int hsize = endpoints_hash_size(lid.beams);
    size_t ep_lds = (size_t)(2 * hsize + 32 + (mark ? 6 * lv.tmax * ((lv.tmax + 31) / 32) + (lv.tmax * lv.tmax + 31) / 32 : 0)) * sizeof(int);
    const int G = lv.ep_group > 0 ? lv.ep_group : 1;
    const int nt = lid.beams <= 192 ? 192 : 256;
    // round 4: only the tiles the poses read are marked, not the wider region the block minima of the bounds summarise (see
    // k_endpoints: 13 % fewer needed tiles, 6 % fewer blurred ones at config 2, the same surviving pose tiles)
    // own_frame_maps: the frame's duties and the occupied-cell scatter as further blocks of this launch
    const bool with_scatter = own_frame_maps != nullptr;
    const int sbx = with_scatter ? cdiv(cdiv(lv.wmax, 32) + 1, 64) : 0, sby = with_scatter ? cdiv(lv.wmax, (nt / 64) * SCATTER_ROLE_NR) : 0;
    if (with_scatter) ep_lds = ep_lds > (size_t)lv.wmax * sizeof(int32_t) ? ep_lds : (size_t)lv.wmax * sizeof(int32_t);
    const dim3 grid(cdiv(lv.ntheta, G) + (own_frame_maps ? 2 : 1) + sbx * sby, P);
    if (nt == 192)
        k_endpoints<192><<<grid, 192, ep_lds, s>>>(lid, lv, d_est, est_stride, d_ranges, d_flags, est_moving_dist, lv.fine ? nullptr : d_psi_cs,
                                                   mark ? 1 : 0, prune ? 1 : 0, beam_table && lv.beam_xy ? 1 : 0, own_frame_maps, sbx);
    else
        k_endpoints<256><<<grid, 256, ep_lds, s>>>(lid, lv, d_est, est_stride, d_ranges, d_flags, est_moving_dist, lv.fine ? nullptr : d_psi_cs,
                                                   mark ? 1 : 0, prune ? 1 : 0, beam_table && lv.beam_xy ? 1 : 0, own_frame_maps, sbx);
}

// cube sweep + selection
// k_bound_lds where the level carries the byte image of the bounds (Slam2dLevel.gmin2b) and it fits the CU's LDS.
// SLAM2D_BOUND_LDS=0: never.  A particle's angles are split over up to BOUND_LDS_MAX_SPLIT blocks (each stages the image)
// while the launch stays below BOUND_LDS_BLOCKS blocks (128: measured at 16 / 64 / 128 / 256 particles per launch, four /
// two / one / one block per particle): small launches need the CUs, large ones pay for every extra staging pass and barrier.
#define BOUND_LDS_MAX_SPLIT 4
#define BOUND_LDS_BLOCKS 128
#define BOUND_LDS_BLOCKS_RLE 256     // long lists: an angle is 16 us of one wave (config 5's 64-particle launches, 139 angles, four blocks per particle)
// The one predicate "this level's bounds will be computed by k_bound_lds", with the launch's shape: made once per slam2d_match,
// read by launch_field (which then leaves the refresh of the bound minima to that kernel) and by launch_bound_lds.
static BoundLdsPlan bound_lds_plan(const Slam2dLevel& lv, int P) {
    static const int mode = [] { const char* e = getenv("SLAM2D_BOUND_LDS"); return e ? atoi(e) : -1; }();
    BoundLdsPlan pl{};
    if (mode == 0 || lv.bnb != 1 || !lv.gmin2b) return pl;
    const int nbt = cube_of(lv).nbt;
    pl.nset = cdiv(nbt * nbt, WAVE);
    const int gp = lv.tmax << 2, lp = lv.g2b_pitch;
    if (pl.nset > 4 || lv.kmax > 2048 || lp < gp || (lp & 15)) return pl;
    const size_t image = ((size_t)gp * lp + 15) & ~(size_t)15;
    // run-length lists from SLAM2D_BEAM_TABLE_MIN cells (16-bit offsets in the run words)
    pl.rle = lv.kmax >= SLAM2D_BEAM_TABLE_MIN && image + (size_t)nbt * lp < 65536;
    const int blocks = pl.rle ? BOUND_LDS_BLOCKS_RLE : BOUND_LDS_BLOCKS;
    pl.bpp = max(1, min(min(BOUND_LDS_MAX_SPLIT, lv.ntheta), blocks / max(P, 1)));
    pl.tpb = cdiv(lv.ntheta, pl.bpp);                           // angles per block
    const int rounds = cdiv(pl.tpb, 16);
    pl.nw = cdiv(pl.tpb, rounds);
    pl.lds = image + (pl.rle ? (size_t)pl.nw * WAVE * sizeof(unsigned) : 0);
    if (!pl.rle && pl.nset <= 2) {                              // the first angle's loads hoisted: a list-head slot per wave behind the image
        BoundLdsPlan hp = pl;
        hp.hoist = true;
        hp.lds = image + (size_t)pl.nw * BL_HEAD * sizeof(int);
        if (bound_lds_dispatch(lv, P, hp, false, 0, nullptr)) { hp.ok = true; return hp; }
    }                                                           // (not granted with the slots: the same kernel without them)
    pl.ok = bound_lds_dispatch(lv, P, pl, false, 0, nullptr);      // (the grant alone)
    return pl;
}
// false: nothing launched (the plan says k_bound)
static bool launch_bound_lds(const Slam2dLevel& lv, int P, const BoundLdsPlan& pl, bool refresh, hipStream_t s) {
    return pl.ok && bound_lds_dispatch(lv, P, pl, true, refresh ? 1 : 0, s);
}

static int launch_scores(const Slam2dLevel& lv, int P, const double* d_est, int est_stride, const double* d_uniform,
                         Slam2dMatch* d_out, hipStream_t s, int ring_chunks = 0) {
    const int nslot = cube_slots(lv), chunks = cube_chunks(lv);
    if (lv.ntheta * chunks > lv.npartial) return SLAM2D_E_BADARG;
    if (ring_chunks > 0) {
        // the prior's ring first (write_priors); the particles it does not settle are swept in full by the
        // second pair of launches, whose blocks return at once for everyone else
        {
            StageScope prof(SLAM2D_STAGE_SWEEP, s);
            launch_sweep(lv, P, min(ring_chunks, chunks), s, 1);
        }
        {
            StageScope prof(SLAM2D_STAGE_SELECT, s);
            k_select<1><<<P, WAVE, 0, s>>>(lv, min(ring_chunks, chunks), d_est, est_stride, d_uniform, d_out);
        }
    }
    const int mode = ring_chunks > 0 ? 2 : 0;
    if (mode == 0 && nslot <= 32) {           // small cube: one wave per (particle, theta) plane
        const unsigned grid = (unsigned)cdiv(P, 8) * 8 * lv.ntheta;
        const size_t lds = (size_t)WAVE * 4 * sizeof(unsigned long long) + (size_t)lv.kmax * sizeof(int);
        const int pruned = lv.bnb == 3 ? 1 : 0;
        if (pruned) {                                                     // angle bounds first, then one exact seed per particle
            StageScope prof(SLAM2D_STAGE_BOUND, s);
            k_abound<<<(unsigned)cdiv(P, 8) * 8 * cdiv(lv.ntheta, ABOUND_WAVES), WAVE * ABOUND_WAVES, 0, s>>>(lv, P);
            k_aseed<<<P, WAVE * ASEED_WAVES, (size_t)ASEED_WAVES * WAVE * 4 * sizeof(unsigned long long) + (size_t)lv.kmax * sizeof(int), s>>>(lv, P);
        }
        {
            StageScope prof(SLAM2D_STAGE_SWEEP, s);
            k_sweep_small<<<grid, WAVE, lds, s>>>(lv, P, pruned);
        }
        StageScope prof(SLAM2D_STAGE_SELECT, s);
        k_select<0><<<P, WAVE, 0, s>>>(lv, 1, d_est, est_stride, d_uniform, d_out);
        return 0;
    }
    // a level matched by arg-max (no soft-max draw: the fine level, matchMax) needs nothing of the cube for its selection: the
    // sweep's last block of every particle does it from the partials (k_sweep, sel_out) and k_select is not launched
    const bool fused = mode == 0 && d_uniform == nullptr && lv.sync != nullptr;
    {
        StageScope prof(SLAM2D_STAGE_SWEEP, s);
        launch_sweep(lv, P, chunks, s, mode, fused ? d_est : nullptr, est_stride, fused ? d_out : nullptr);
    }
    if (fused) return 0;
    {
        StageScope prof(SLAM2D_STAGE_SELECT, s);
        if (mode == 0) k_select<0><<<P, WAVE, 0, s>>>(lv, chunks, d_est, est_stride, d_uniform, d_out);
        else k_select<2><<<P, WAVE, 0, s>>>(lv, chunks, d_est, est_stride, d_uniform, d_out);
    }
    return 0;
}

// Upper bound (a superset is harmless) of the number of sweep slots the prior's ring touches, for the grid of
// the ring pass; 0 = pruning not applicable.  The ring itself is listed on the device by write_priors.
static int ring_slot_bound(const Slam2dLevel& lv, double est_dist) {
    if (lv.fine || !lv.ring || !lv.prune_state || lv.ring_cap <= 0 || !(est_dist >= 0.0)) return 0;
    const int nx = cube_of(lv).nx, nq = cube_of(lv).nq;
    const double slack = 1e-9 * (1.0 + est_dist + lv.step * nx);
    int n = 0;
    for (int iy = 0; iy < nx; ++iy)
        for (int sq = 0; sq < nq; ++sq) {
            bool in = false;
            for (int e = 0; e < 4 && 4 * sq + e < nx; ++e) {
                const double mx = (double)(4 * sq + e - lv.ncell) * lv.step, my = (double)(iy - lv.ncell) * lv.step;
                in = in || !(fabs(sqrt(mx * mx + my * my) - est_dist) > lv.max_move_dev + slack);
            }
            n += in ? 1 : 0;
        }
    return n <= lv.ring_cap ? n : 0;
}

// Blocks per particle of k_exact_select: enough to put every CU to work (256 CUs / P particles), at most 4; needs the
// arrival counters (Slam2dLevel.sync).
static int exact_split(const Slam2dLevel& lv, int P) {
    if (!lv.sync) return 1;
    int n = 256 / (P > 0 ? P : 1);      // (the kernel lets only XS_SPLIT_LIGHT of them work on a particle with few tiles)
    if (n > XS_SPLIT_MAX) n = XS_SPLIT_MAX;
    return n < 1 ? 1 : n;
}

int slam2d_field_build(const Slam2dLidar* lidar, const Slam2dLevel* level, const Slam2dMap* d_maps, int32_t P,
                       const double* d_centre, int32_t centre_stride, uint32_t* d_flags, void* stream) {
    int rc = check_level(lidar, level, P);
    if (rc) return rc;
    if (!d_maps || !d_centre || !d_flags || centre_stride < 2) return SLAM2D_E_BADARG;
    { Slam2dLevel chk = *level; chk.bnb = 0; if ((rc = check_field_args(chk, P, false))) return rc; }
    hipStream_t s = (hipStream_t)stream;
    Slam2dLevel lv = *level;
    lv.bnb = 0;                                        // the full build has no pooled image
    if ((rc = launch_frames(*lidar, lv, d_maps, P, d_centre, centre_stride, d_flags, false, s))) return rc;
    if ((rc = launch_field(lv, d_maps, P, d_flags, false, s))) return rc;
    return launch_status();
}

int slam2d_field_build_distance(const Slam2dLidar* lidar, const Slam2dLevel* level, const Slam2dMap* d_maps, int32_t P,
                                const double* d_centre, int32_t centre_stride, const uint32_t* d_lut, int32_t lut_n,
                                uint32_t* d_dist2, uint32_t* d_flags, void* stream) {
    int rc = check_level(lidar, level, P);
    if (rc) return rc;
    if (!d_maps || !d_centre || !d_flags || centre_stride < 2) return SLAM2D_E_BADARG;
    if (!d_lut || lut_n < 1 || lut_n > SLAM2D_DISTANCE_MAX_TABLE) return SLAM2D_E_BADARG;
    if (!level->frames || !level->axis_x || !level->axis_y || !level->field) return SLAM2D_E_BADARG;
    if (level->occ_gen < 0 || level->occ_gen > 255) return SLAM2D_E_BADARG;
    { Slam2dLevel chk = *level; chk.bnb = 0; if ((rc = check_field_args(chk, P, false))) return rc; }
    hipStream_t s = (hipStream_t)stream;
    Slam2dLevel lv = *level;
    lv.bnb = 0;                                        // as the full build: no pooled image
    if ((rc = launch_frames(*lidar, lv, d_maps, P, d_centre, centre_stride, d_flags, false, s))) return rc;
    launch_scatter(lv, d_maps, P, s);
    const int cap = lut_n - 1;
    int R = 0;
    while (R * R < cap) ++R;                           // ceil(sqrt(cap)) <= 256
    const int S = max(R, 32);                          // rows per thread of the column pass: it reads up to S + 2 R
    k_dist_cols<<<dim3(cdiv(lv.fmax, 256), cdiv(lv.fmax, S), P), 256, 0, s>>>(lv, R, S);
    k_dist_rows<<<dim3(lv.fmax, P), 256, ((size_t)lv.fmax * sizeof(uint16_t) + 15) & ~(size_t)15, s>>>(lv, d_lut, cap, R, d_dist2);
    // the slots no longer hold what slam2d_field_build left there (SearchLevel.set_field on the host)
    const size_t ntile = (size_t)lv.tmax * lv.tmax;
    if ((rc = (int)hipMemsetAsync(lv.tilestate, 1, (size_t)P * ntile, s))) return rc;
    if (lv.freerow && (rc = (int)hipMemsetAsync(lv.freerow, 0, (size_t)P * 64 * sizeof(unsigned long long), s))) return rc;
    return launch_status();
}

int slam2d_sweep(const Slam2dLidar* lidar, const Slam2dLevel* level, int32_t P, const double* d_est,
                 int32_t est_stride, const double* d_ranges, double est_moving_dist, const double* d_psi_cs,
                 const double* d_uniform, Slam2dMatch* d_out, uint32_t* d_flags, void* stream) {
    int rc = check_level(lidar, level, P);
    if (rc) return rc;
    if (!d_est || !d_ranges || !d_out || !d_flags || est_stride < 3) return SLAM2D_E_BADARG;
    Slam2dLevel lv = *level;
    lv.bnb = 0;                                        // the whole cube, brute force
    if (lv.kmax < lidar->beams || !lv.partials) return SLAM2D_E_BADARG;
    hipStream_t s = (hipStream_t)stream;
    launch_endpoints(*lidar, lv, P, d_est, est_stride, d_ranges, est_moving_dist, d_psi_cs, d_flags, false, false, s);
    if ((rc = launch_scores(lv, P, d_est, est_stride, d_uniform, d_out, s))) return rc;
    return launch_status();
}

int slam2d_match(const Slam2dLidar* lidar, const Slam2dLevel* level, const Slam2dMap* d_maps, int32_t P,
                 const double* d_est, int32_t est_stride, const double* d_ranges, double est_moving_dist,
                 const double* d_psi_cs, const double* d_uniform, Slam2dMatch* d_out, uint32_t* d_flags,
                 uint32_t options, void* stream) {
    int rc = check_level(lidar, level, P);
    if (rc) return rc;
    if (!d_maps || !d_est || !d_ranges || !d_out || !d_flags || est_stride < 3) return SLAM2D_E_BADARG;
    const Slam2dLevel& lv = *level;
    if (lv.kmax < lidar->beams || !lv.partials) return SLAM2D_E_BADARG;
    if ((rc = check_field_args(lv, P, true))) return rc;
    hipStream_t s = (hipStream_t)stream;
    int ring_chunks = 0;
    if (options & SLAM2D_MATCH_PRUNE_BY_PRIOR) {
        const int bound = ring_slot_bound(lv, est_moving_dist);
        if (bound > 0 && 2 * bound <= cube_slots(lv)) ring_chunks = cdiv(bound, WAVE);     // worth it only for a thin ring
    }
    // Below SLAM2D_BEAM_TABLE_MIN beams k_frame_axis is not launched at all: the endpoint kernel's per-particle block does
    // its work (one launch less per level) and the occupied-cell scatter rides in that launch as well; above, and from
    // SLAM2D_FRAME_KERNEL_MIN_P particles per launch, k_frame_axis also tabulates the beam endpoints once per particle.
    const bool framed = lidar->beams >= SLAM2D_BEAM_TABLE_MIN || lv.occ_gen == 0 || P >= SLAM2D_FRAME_KERNEL_MIN_P;
    const Slam2dMap* own = framed ? nullptr : d_maps;
    if (lv.occ_gen < 0 || lv.occ_gen > 255) return SLAM2D_E_BADARG;
    if (lv.bnb && lv.bnb != 3) {
        // branch and bound over 4x4 pose tiles: tile bounds + seed tiles, surviving tiles + selection
        if (framed && (rc = launch_frames(*lidar, lv, d_maps, P, d_est, est_stride, d_flags, true, s, d_ranges))) return rc;
        launch_endpoints(*lidar, lv, P, d_est, est_stride, d_ranges, est_moving_dist, d_psi_cs, d_flags, true, false, s, framed, own);
        // (nothing here reads the field's maximum: that is the prior pruning's, which scores by the sweep)
        const BoundLdsPlan plan = bound_lds_plan(lv, P);
        const bool refresh = fold_field_check(lv, true, false, plan.ok);     // launch_field's own decision: k_bound_lds refreshes the bound minima
        if ((rc = launch_field(lv, d_maps, P, d_flags, true, s, !framed, false, plan.ok))) return rc;
        const unsigned grid = (unsigned)cdiv(P, 8) * 8 * lv.ntheta;
        if (lv.bnb == 2) {
            StageScope prof(SLAM2D_STAGE_BOUND, s);
            k_bound1<<<grid, WAVE, (size_t)(WAVE * 4 + lv.kmax) * sizeof(int), s>>>(lv, P);
            k_seed<<<P, SEED_THREADS, 0, s>>>(lv, P);
            k_bound2<<<grid, WAVE, 0, s>>>(lv, P);
        } else {
            StageScope prof(SLAM2D_STAGE_BOUND, s);
            if (!launch_bound_lds(lv, P, plan, refresh, s)) {
                if (refresh) return SLAM2D_E_BADARG;       // (cannot happen: the fold read the same plan) never k_bound on stale minima
                k_bound<<<(unsigned)cdiv(P, 8) * 8 * cdiv(lv.ntheta, BOUND_GROUP), WAVE * BOUND_GROUP, 0, s>>>(lv, P);
            }
        }
        {
            StageScope prof(SLAM2D_STAGE_EXACT, s);
            const int nsplit = exact_split(lv, P);
            if (nsplit > 1) k_exact_select<true><<<(unsigned)cdiv(P, 8) * 8 * nsplit, XS_THREADS, 0, s>>>(lv, d_est, est_stride, d_uniform, d_out, P, nsplit);
            else k_exact_select<false><<<P, XS_THREADS, 0, s>>>(lv, d_est, est_stride, d_uniform, d_out, P, 1);
        }
        return launch_status();
    }
    // the endpoints need only the frame, so they run first and tell the field build which tiles matter
    if (framed && (rc = launch_frames(*lidar, lv, d_maps, P, d_est, est_stride, d_flags, true, s, d_ranges))) return rc;
    launch_endpoints(*lidar, lv, P, d_est, est_stride, d_ranges, est_moving_dist, d_psi_cs, d_flags, true, ring_chunks > 0, s, framed, own);
    if ((rc = launch_field(lv, d_maps, P, d_flags, true, s, !framed, ring_chunks > 0))) return rc;      // (the ring pass reads the field's maximum)
    if ((rc = launch_scores(lv, P, d_est, est_stride, d_uniform, d_out, s, ring_chunks))) return rc;
    return launch_status();
}

static int check_moments_level(const Slam2dLevel* lv, int P) {
    if (!lv || P <= 0) return SLAM2D_E_BADARG;
    if (lv->fmax <= 0 || lv->fpitch < lv->fmax || lv->ncell < 0 || lv->ntheta <= 0 || lv->kmax <= 0 || !(lv->cost_scale > 0.0)) return SLAM2D_E_BADARG;
    if ((long long)lv->fmax * lv->fpitch >= (1ll << 29)) return SLAM2D_E_TOOLARGE;     // byte offsets into one field stay below 2^31
    const long long nx = 2ll * lv->ncell + 1;
    if (nx > 4096 || (long long)lv->ntheta * nx * nx >= (1ll << 31)) return SLAM2D_E_TOOLARGE;      // flat pose indices are int32
    return 0;
}

int64_t slam2d_match_moments_work(const Slam2dLevel* level, int32_t P) {
    const int rc = check_moments_level(level, P);
    if (rc) return rc;
    return (int64_t)P * level->ntheta * cube_chunks(*level) * MOMENTS_ROW;
}

int slam2d_match_moments(const Slam2dLevel* level, int32_t P, const double* d_est, int32_t est_stride,
                         const Slam2dMatch* d_match, double* d_work, double* d_out, void* stream) {
    if (!d_est || !d_match || !d_work || !d_out || est_stride < 3) return SLAM2D_E_BADARG;
    const int rc = check_moments_level(level, P);
    if (rc) return rc;
    const Slam2dLevel& lv = *level;
    if (!lv.field || !lv.cells || !lv.kcount || !lv.prior || !lv.thetas) return SLAM2D_E_BADARG;
    hipStream_t s = (hipStream_t)stream;
    const int chunks = cube_chunks(lv);
    const int bpp = lv.ntheta * chunks;                                 // blocks (= rows of d_work) per particle
    if ((long long)cdiv(P, 8) * 8 * bpp >= (1ll << 31)) return SLAM2D_E_TOOLARGE;
    k_moments<<<(unsigned)cdiv(P, 8) * 8 * bpp, 256, 0, s>>>(lv, P, chunks, bpp, d_match, d_work);
    k_moments_fold<<<P, WAVE, 0, s>>>(lv, bpp, d_match, d_work, d_out);
    return launch_status();
}

// The lidar tables every spoke walk reads (k_grid_update, k_occ_extent, k_map_scans, k_predict_scan).  need_table: the kernel reads
// lut_xs itself; the others take the window coordinates from lut_xs_step where it is set (window_coord).  The negated form refuses
// a NaN unit.  The beam count is each entry point's own check: their codes differ.
static int check_spoke_lidar(const Slam2dLidar* lidar, const bool need_table) {
    if (!lidar || !lidar->spoke_band || !lidar->spoke_cells || !lidar->spoke_r) return SLAM2D_E_BADARG;
    if (lidar->num_bands < 1 || lidar->num_spokes < 1 || lidar->lut_w < 2 || lidar->lut_w > 65535 || !(lidar->unit > 0.0)) return SLAM2D_E_BADARG;
    if (!lidar->lut_xs && (need_table || lidar->lut_xs_step == 0.0)) return SLAM2D_E_BADARG;
    return 0;
}

static int launch_update(const Slam2dLidar* lidar, const Slam2dMap* d_maps, int32_t P, const double* d_pose, int32_t pose_stride,
                         const double* d_ranges, const int32_t* d_beam_shift, uint32_t* d_flags, const WeightsJob& wj, void* stream) {
    if (!d_maps || !d_pose || !d_ranges || !d_flags || P <= 0 || pose_stride < 3 || check_spoke_lidar(lidar, false)) return SLAM2D_E_BADARG;
    if (lidar->beams < 1 || lidar->beams > SLAM2D_MAX_BEAMS) return SLAM2D_E_TOOLARGE;
    hipStream_t s = (hipStream_t)stream;
    const int groups = cdiv(lidar->beams, UPDB_BEAMS);
    StageScope prof(SLAM2D_STAGE_UPDATE, s);
    k_grid_update<<<8 * cdiv(P, 8) * groups + (wj.logw ? 1 : 0), 64 * UPDB_BEAMS, 0, s>>>(*lidar, d_maps, P, d_pose, pose_stride, d_ranges,
                                                                                         d_beam_shift, d_flags, groups, wj);
    return launch_status();
}

int slam2d_grid_update(const Slam2dLidar* lidar, const Slam2dMap* d_maps, int32_t P, const double* d_pose,
                       int32_t pose_stride, const double* d_ranges, const int32_t* d_beam_shift, uint32_t* d_flags,
                       void* stream) {
    return launch_update(lidar, d_maps, P, d_pose, pose_stride, d_ranges, d_beam_shift, d_flags, WeightsJob{}, stream);
}

int slam2d_occ_extent(const Slam2dLidar* lidar, int32_t S, const double* d_pose, int32_t pose_stride, const double* d_ranges,
                      double* d_out, void* stream) {
    if (!d_pose || !d_ranges || !d_out || S <= 0 || pose_stride < 3 || check_spoke_lidar(lidar, true)) return SLAM2D_E_BADARG;
    if (lidar->beams < 1 || lidar->beams > SLAM2D_MAX_BEAMS) return SLAM2D_E_TOOLARGE;
    const int groups = cdiv(lidar->beams, MAPS_BEAMS);
    if ((long long)S * groups > 0x7fffffffll) return SLAM2D_E_TOOLARGE;
    k_occ_extent<<<S * groups, 64 * MAPS_BEAMS, 0, (hipStream_t)stream>>>(*lidar, S, groups, d_pose, pose_stride, d_ranges, d_out);
    return launch_status();
}

int slam2d_map_scans(const Slam2dLidar* lidar, const Slam2dMap* d_map, int32_t S, const double* d_pose, int32_t pose_stride,
                     const double* d_ranges, const Slam2dBeamPlan* d_plan, const uint16_t* d_lut_bin, const double* d_lut_r,
                     uint32_t* d_flags, void* stream) {
    if (!d_map || !d_pose || !d_ranges || !d_plan || !d_lut_bin || !d_lut_r || !d_flags || S <= 0 || pose_stride < 3 ||
        check_spoke_lidar(lidar, true))
        return SLAM2D_E_BADARG;
    if (lidar->beams < 1 || lidar->beams > SLAM2D_MAX_BEAMS) return SLAM2D_E_TOOLARGE;
    const int groups = cdiv(lidar->beams, MAPS_BEAMS);
    if ((long long)S * groups > 0x7fffffffll) return SLAM2D_E_TOOLARGE;
    k_map_scans<<<S * groups, 64 * MAPS_BEAMS, 0, (hipStream_t)stream>>>(*lidar, d_map, S, groups, d_pose, pose_stride, d_ranges, d_plan, d_lut_bin,
                                                        d_lut_r, d_flags);
    return launch_status();
}

int slam2d_predict_scan(const Slam2dLidar* lidar, const Slam2dMap* d_maps, int32_t map_stride, int32_t S, const double* d_pose,
                        int32_t pose_stride, double r_min, double r_max, double* d_out, void* stream) {
    if (!d_maps || !d_pose || !d_out || S <= 0 || pose_stride < 3 || (map_stride != 0 && map_stride != 1) || check_spoke_lidar(lidar, false))
        return SLAM2D_E_BADARG;
    if (lidar->beams <= 0 || lidar->beams > SLAM2D_MAX_BEAMS) return SLAM2D_E_BADARG;
    if (!(r_min >= 0.0) || !(r_max > r_min)) return SLAM2D_E_BADARG;              // (the negated forms refuse a NaN)
    const int groups = cdiv(lidar->beams, MAPS_BEAMS);
    if ((long long)S * groups > 0x7fffffffll) return SLAM2D_E_TOOLARGE;
    k_predict_scan<<<S * groups, 64 * MAPS_BEAMS, 0, (hipStream_t)stream>>>(*lidar, d_maps, map_stride, S, groups, d_pose, pose_stride,
                                                                            r_min, r_max, d_out);
    return launch_status();
}

// What every call of this layer asks of the level whose slot p_field it reads (no lidar is read).  Every SLAM2D_E_BADARG comes
// before any SLAM2D_E_TOOLARGE, so a caller returns the former at once and the latter after its own argument checks.
static int check_level_field(const Slam2dLevel* level, int p_field) {
    if (!level || !level->field || !level->frames || p_field < 0) return SLAM2D_E_BADARG;
    if (!(level->step > 0.0) || !(level->cost_scale > 0.0)) return SLAM2D_E_BADARG;                  // (the negated forms refuse a NaN)
    // the field's limits as check_level has them: a cell key packs (row << 16 | column), offsets into one image stay below 2^31
    if (level->fmax <= 0 || level->fpitch < level->fmax) return SLAM2D_E_BADARG;
    if ((long long)level->fmax * level->fpitch >= (1ll << 29)) return SLAM2D_E_TOOLARGE;
    return 0;
}
// The same for the calls that score a scan: the lidar's checks, all of them SLAM2D_E_BADARG, in front
static int check_scored_field(const Slam2dLidar* lidar, const Slam2dLevel* level, int p_field) {
    if (!lidar || lidar->beams < 1 || lidar->beams > SLAM2D_MAX_BEAMS || !(lidar->max_range > 0.0)) return SLAM2D_E_BADARG;
    return check_level_field(level, p_field);
}

int slam2d_score_poses(const Slam2dLidar* lidar, const Slam2dLevel* level, int32_t p_field, int32_t N, const double* d_pose,
                       int32_t pose_stride, const double* d_ranges, int32_t ranges_stride, double* d_out, void* stream) {
    const int rc = check_scored_field(lidar, level, p_field);
    if (rc == SLAM2D_E_BADARG) return rc;
    if (!d_pose || !d_ranges || !d_out || N <= 0 || pose_stride < 3) return SLAM2D_E_BADARG;
    if (ranges_stride != 0 && ranges_stride < lidar->beams) return SLAM2D_E_BADARG;
    if (rc) return rc;
    const int hsize = score_hash_size(lidar->beams);
    const int waves = hsize > 2048 ? SCORE_WAVES / 2 : SCORE_WAVES;               // <= 32 KB of hash sets per block
    const long long blocks = ((long long)N + waves - 1) / waves;
    if (blocks * (64 * waves) > 0xffffffffll) return SLAM2D_E_TOOLARGE;           // (a launch holds fewer than 2^32 threads)
    k_score_poses<<<(unsigned)blocks, 64 * waves, (size_t)waves * hsize * sizeof(int), (hipStream_t)stream>>>(
        *lidar, *level, p_field, N, hsize, d_pose, pose_stride, d_ranges, ranges_stride, d_out);
    return launch_status();
}

int slam2d_score_points(const Slam2dLevel* level, int32_t p_field, int32_t N, const double* d_pose, int32_t pose_stride, const double* d_points,
                        int32_t point_stride, int32_t M, int32_t set_stride, double* d_out, void* stream) {
    const int rc = check_level_field(level, p_field);
    if (rc == SLAM2D_E_BADARG) return rc;
    if (!d_pose || !d_points || !d_out || N <= 0 || pose_stride < 3) return SLAM2D_E_BADARG;
    if (M < 1 || M > SLAM2D_MAX_POINTS || point_stride < 2) return SLAM2D_E_BADARG;
    if (set_stride != 0 && (long long)set_stride < (long long)M * point_stride) return SLAM2D_E_BADARG;
    if (rc) return rc;
    const int hsize = score_hash_size(M);
    const int waves = hsize > 2048 ? SCORE_WAVES / 2 : SCORE_WAVES;               // <= 32 KB of hash sets per block
    const long long blocks = ((long long)N + waves - 1) / waves;
    if (blocks * (64 * waves) > 0xffffffffll) return SLAM2D_E_TOOLARGE;           // (a launch holds fewer than 2^32 threads)
    k_score_points<<<(unsigned)blocks, 64 * waves, (size_t)waves * hsize * sizeof(int), (hipStream_t)stream>>>(
        *level, p_field, N, hsize, d_pose, pose_stride, d_points, point_stride, M, set_stride, d_out);
    return launch_status();
}

// What the two ray calls ask of their lidar and level (they read beams, fov, max_range; frames, step, fmax, fpitch): every
// SLAM2D_E_BADARG in front of the one SLAM2D_E_TOOLARGE, as in check_level_field
static int check_ray_field(const Slam2dLidar* lidar, const Slam2dLevel* level, int p_field) {
    if (!lidar || lidar->beams < 1 || lidar->beams > SLAM2D_MAX_BEAMS || !(lidar->max_range > 0.0)) return SLAM2D_E_BADARG;
    if (!level || !level->frames || p_field < 0 || !(level->step > 0.0)) return SLAM2D_E_BADARG;   // (the negated forms refuse a NaN)
    if (level->fmax <= 0 || level->fpitch < level->fmax) return SLAM2D_E_BADARG;
    if ((long long)level->fmax * level->fpitch >= (1ll << 29)) return SLAM2D_E_TOOLARGE;
    return 0;
}

int slam2d_cast_rays(const Slam2dLidar* lidar, const Slam2dLevel* level, int32_t p_field, const uint32_t* d_dist2, int32_t N,
                     const double* d_pose, int32_t pose_stride, int32_t K, uint32_t* d_out, void* stream) {
    const int rc = check_ray_field(lidar, level, p_field);
    if (rc == SLAM2D_E_BADARG) return rc;
    if (!d_dist2 || !d_pose || !d_out || N <= 0 || pose_stride < 3 || K < 0) return SLAM2D_E_BADARG;
    if (rc) return rc;
    if (K >= SLAM2D_RAY_MAX_K) return SLAM2D_E_TOOLARGE;
    const int groups = cdiv(lidar->beams, 64);
    const long long blocks = ((long long)N * groups + RAY_WAVES - 1) / RAY_WAVES;
    if (blocks * (64 * RAY_WAVES) > 0xffffffffll) return SLAM2D_E_TOOLARGE;       // (a launch holds fewer than 2^32 threads)
    k_cast_rays<<<(unsigned)blocks, 64 * RAY_WAVES, 0, (hipStream_t)stream>>>(*lidar, *level, p_field, d_dist2, N, groups, d_pose, pose_stride, K,
                                                                              d_out);
    return launch_status();
}

int slam2d_score_rays(const Slam2dLidar* lidar, const Slam2dLevel* level, int32_t p_field, const uint32_t* d_dist2, int32_t N,
                      const double* d_pose, int32_t pose_stride, const double* d_ranges, int32_t ranges_stride, int32_t margin,
                      uint32_t outside_cost, uint32_t through_cost, double* d_out, void* stream) {
    const int rc = check_ray_field(lidar, level, p_field);
    if (rc == SLAM2D_E_BADARG) return rc;
    if (!level->field || !d_dist2 || !d_pose || !d_ranges || !d_out || N <= 0 || pose_stride < 3 || margin < 0) return SLAM2D_E_BADARG;
    if (ranges_stride != 0 && ranges_stride < lidar->beams) return SLAM2D_E_BADARG;
    if (rc) return rc;
    const long long blocks = ((long long)N + RAY_WAVES - 1) / RAY_WAVES;
    if (blocks * (64 * RAY_WAVES) > 0xffffffffll) return SLAM2D_E_TOOLARGE;       // (a launch holds fewer than 2^32 threads)
    k_score_rays<<<(unsigned)blocks, 64 * RAY_WAVES, 0, (hipStream_t)stream>>>(*lidar, *level, p_field, d_dist2, N, d_pose, pose_stride, d_ranges,
                                                                               ranges_stride, margin, outside_cost, through_cost, d_out);
    return launch_status();
}

// the checks slam2d_search_lattice and its work size share; *words: the 8-byte words of d_work (the endpoint table)
static int check_search_lattice(const Slam2dLidar* lidar, int nx, int ny, int nth, long long* words) {
    if (!lidar || nx < 1 || ny < 1 || nth < 1 || nth > 65536) return SLAM2D_E_BADARG;
    if (lidar->beams < 1 || lidar->beams > SLAM2D_MAX_BEAMS) return SLAM2D_E_BADARG;
    if ((long long)nx * ny >= (1ll << 31)) return SLAM2D_E_TOOLARGE;
    *words = 2ll * nth * lidar->beams;                                            // (at most 2^28)
    if (*words > (1ll << 31)) return SLAM2D_E_TOOLARGE;
    return 0;
}

int64_t slam2d_search_lattice_work(const Slam2dLidar* lidar, int32_t nx, int32_t ny, int32_t nth) {
    long long words = 0;
    const int rc = check_search_lattice(lidar, nx, ny, nth, &words);
    return rc ? rc : words;
}

// The launch geometry of the two lattice searches: a thread per position, a block row per hc headings.  (Heading chunks exist
// only below SEARCH_WAVES waves of positions, at most 8192 of them: the launch stays below 2^32 threads.)
struct SearchGrid { int positions, hc; long long blocks, rows; };
static SearchGrid search_grid(int nx, int ny, int nth) {
    const int positions = nx * ny, hc = search_chunk(positions, nth);
    return SearchGrid{positions, hc, ((long long)positions + 255) / 256, cdiv(nth, hc)};
}

int slam2d_search_lattice(const Slam2dLidar* lidar, const Slam2dLevel* level, int32_t p_field, int32_t nx, int32_t ny, int32_t nth,
                          double x0, double dx, double y0, double dy, double th0, double dth, const double* d_ranges,
                          uint32_t outside_cost, uint64_t* d_work, uint64_t* d_out, void* stream) {
    const int frc = check_scored_field(lidar, level, p_field);
    if (frc == SLAM2D_E_BADARG) return frc;
    if (!d_ranges || !d_out) return SLAM2D_E_BADARG;
    if (!__builtin_isfinite(dx) || !__builtin_isfinite(dy) || !__builtin_isfinite(dth)) return SLAM2D_E_BADARG;
    long long words = 0;
    const int rc = check_search_lattice(lidar, nx, ny, nth, &words);
    if (rc == SLAM2D_E_BADARG) return rc;
    if (words > 0 && !d_work) return SLAM2D_E_BADARG;
    if (rc) return rc;
    if (frc) return frc;
    const SearchGrid g = search_grid(nx, ny, nth);
    hipStream_t s = (hipStream_t)stream;
    double2* E = reinterpret_cast<double2*>(d_work);
    const long long first = g.positions > words / 2 ? g.positions : words / 2;
    k_search_table<<<(unsigned)((first + 255) / 256), 256, 0, s>>>(*lidar, nth, th0, dth, d_ranges, E, (unsigned long long*)d_out, g.positions);
    k_search_lattice<<<dim3((unsigned)g.blocks, (unsigned)g.rows), 256, 0, s>>>(*lidar, *level, p_field, nx, g.positions, nth, g.hc, x0, dx, y0, dy,
                                                                               d_ranges, E, outside_cost, (unsigned long long*)d_out);
    return launch_status();
}

int64_t slam2d_refine_work(int32_t N) {
    if (N < 1) return SLAM2D_E_BADARG;
    if (N > SLAM2D_REFINE_MAX_BLOCKS) return SLAM2D_E_TOOLARGE;
    return 3ll * N;                                                               // the moved seeds; the join is on d_out itself
}

// The window of the two refinement calls (N >= 1 seeds, `items` table entries per heading: beams or points): radii to the
// lattice, the headings per block row and the rows.  Every SLAM2D_E_BADARG comes before any SLAM2D_E_TOOLARGE.
struct RefineWindow { RefineLattice lat; int hc; long long rows; };
static int check_refine_window(int N, int items, int rx, int ry, int rt, double dx, double dy, double dth, const double* motion, RefineWindow* w) {
    if (rx < 0 || ry < 0 || rt < 0) return SLAM2D_E_BADARG;
    if (!__builtin_isfinite(dx) || !__builtin_isfinite(dy) || !__builtin_isfinite(dth)) return SLAM2D_E_BADARG;
    for (int i = 0; motion && i < 3; ++i)
        if (!__builtin_isfinite(motion[i])) return SLAM2D_E_BADARG;
    const long long nx = 2ll * rx + 1, ny = 2ll * ry + 1, nth = 2ll * rt + 1;     // (each below 2^32)
    if (nx > SLAM2D_REFINE_MAX_CANDIDATES || nx * ny > SLAM2D_REFINE_MAX_CANDIDATES || nx * ny * nth > SLAM2D_REFINE_MAX_CANDIDATES)
        return SLAM2D_E_TOOLARGE;
    w->lat = RefineLattice{(int)nx, (int)ny, (int)nth, dx, dy, dth};
    w->hc = refine_chunk(N, (int)nth, items);
    w->rows = (nth + w->hc - 1) / w->hc;
    if (N > SLAM2D_REFINE_MAX_BLOCKS || N * w->rows > SLAM2D_REFINE_MAX_BLOCKS) return SLAM2D_E_TOOLARGE;    // (256 threads each: below 2^32)
    return 0;
}
// The three launches of a refinement: the move, the given search launch -- search(blocks, moved, out) -- and the winners' poses
extern "C++" template <class Search>
static int launch_refine(int N, const double* d_pose_in, double* d_pose_out, int pose_stride, const double* motion, const RefineWindow& w,
                         uint64_t* d_work, uint64_t* d_out, hipStream_t s, Search search) {
    double* moved = reinterpret_cast<double*>(d_work);
    unsigned long long* out = (unsigned long long*)d_out;
    k_refine_move<<<cdiv(N, 256), 256, 0, s>>>(N, d_pose_in, pose_stride, motion != nullptr, motion ? motion[0] : 0.0, motion ? motion[1] : 0.0,
                                               motion ? motion[2] : 0.0, moved, out);
    search((unsigned)(N * w.rows), moved, out);
    k_refine_pose<<<cdiv(N, 256), 256, 0, s>>>(N, w.lat, moved, out, d_pose_out, pose_stride);
    return launch_status();
}

int slam2d_refine_poses(const Slam2dLidar* lidar, const Slam2dLevel* level, int32_t p_field, int32_t N, const double* d_pose_in,
                        double* d_pose_out, int32_t pose_stride, const double* d_ranges, int32_t ranges_stride, const double motion[3],
                        int32_t rx, int32_t ry, int32_t rt, double dx, double dy, double dth, uint32_t outside_cost, uint64_t* d_work,
                        uint64_t* d_out, void* stream) {
    const int frc = check_scored_field(lidar, level, p_field);
    if (frc == SLAM2D_E_BADARG) return frc;
    if (!d_pose_in || !d_pose_out || !d_ranges || !d_out || !d_work || d_pose_in == d_pose_out) return SLAM2D_E_BADARG;
    if (N < 1 || pose_stride < 3 || (ranges_stride != 0 && ranges_stride < lidar->beams)) return SLAM2D_E_BADARG;
    RefineWindow w;
    const int wrc = check_refine_window(N, lidar->beams, rx, ry, rt, dx, dy, dth, motion, &w);
    if (wrc) return wrc;
    if (frc) return frc;
    hipStream_t s = (hipStream_t)stream;
    return launch_refine(N, d_pose_in, d_pose_out, pose_stride, motion, w, d_work, d_out, s, [&](unsigned blocks, double* moved, unsigned long long* out) {
        k_refine_search<<<blocks, 256, 0, s>>>(*lidar, *level, p_field, (int)w.rows, w.hc, w.lat, moved, d_ranges, ranges_stride, outside_cost, out);
    });
}

int64_t slam2d_refine_rays_work(int32_t N) { return slam2d_refine_work(N); }

int slam2d_refine_poses_rays(const Slam2dLidar* lidar, const Slam2dLevel* level, int32_t p_field, const uint32_t* d_dist2, int32_t N,
                             const double* d_pose_in, double* d_pose_out, int32_t pose_stride, const double* d_ranges, int32_t ranges_stride,
                             const double motion[3], int32_t rx, int32_t ry, int32_t rt, double dx, double dy, double dth, uint32_t outside_cost,
                             int32_t ray_stride, int32_t ray_phase, int32_t margin, uint32_t through_cost, uint32_t* d_through, uint64_t* d_work,
                             uint64_t* d_out, void* stream) {
    const int frc = check_scored_field(lidar, level, p_field);
    if (frc == SLAM2D_E_BADARG) return frc;
    if (!d_dist2 || !d_pose_in || !d_pose_out || !d_ranges || !d_out || !d_work || d_pose_in == d_pose_out) return SLAM2D_E_BADARG;
    if (N < 1 || pose_stride < 3 || (ranges_stride != 0 && ranges_stride < lidar->beams)) return SLAM2D_E_BADARG;
    if (ray_stride < 1 || ray_stride > SLAM2D_MAX_BEAMS || ray_phase < 0 || ray_phase >= ray_stride || margin < 0) return SLAM2D_E_BADARG;
    RefineWindow w;
    const int wrc = check_refine_window(N, lidar->beams, rx, ry, rt, dx, dy, dth, motion, &w);   // (the search's blocks; the last launch has N / 4)
    if (wrc) return wrc;
    if (frc) return frc;
    hipStream_t s = (hipStream_t)stream;
    double* moved = reinterpret_cast<double*>(d_work);
    unsigned long long* out = (unsigned long long*)d_out;
    const RefineRays rays{ray_stride, ray_phase, margin, through_cost};
    const size_t lds = refine_rays_lds_bytes(w.hc, lidar->beams, refine_rays_cast(lidar->beams, ray_stride, ray_phase));
    static size_t granted[64] = {};
    if (!grant_dynamic_lds(reinterpret_cast<const void*>(k_refine_search_rays), granted, lds)) return SLAM2D_E_TOOLARGE;     // (above 64 KiB: asked for once)
    k_refine_move<<<cdiv(N, 256), 256, 0, s>>>(N, d_pose_in, pose_stride, motion != nullptr, motion ? motion[0] : 0.0, motion ? motion[1] : 0.0,
                                               motion ? motion[2] : 0.0, moved, out);
    k_refine_search_rays<<<(unsigned)(N * w.rows), 256, lds, s>>>(*lidar, *level, p_field, d_dist2, (int)w.rows, w.hc, w.lat, moved, d_ranges,
                                                                ranges_stride, outside_cost, rays, out);
    if (d_through)
        k_refine_pose_rays<<<cdiv(N, REFINE_RAYS_WAVES), 64 * REFINE_RAYS_WAVES, 0, s>>>(*lidar, *level, p_field, d_dist2, N, w.lat, moved, d_ranges,
                                                                                         ranges_stride, rays, out, d_pose_out, pose_stride, d_through);
    else
        k_refine_pose<<<cdiv(N, 256), 256, 0, s>>>(N, w.lat, moved, out, d_pose_out, pose_stride);
    return launch_status();
}

// the checks slam2d_search_points and its work size share; *words: the 8-byte words of d_work (the offset table)
static int check_search_points(int M, int nx, int ny, int nth, long long* words) {
    if (M < 1 || M > SLAM2D_MAX_POINTS || nx < 1 || ny < 1 || nth < 1 || nth > 65536) return SLAM2D_E_BADARG;
    if ((long long)nx * ny >= (1ll << 31)) return SLAM2D_E_TOOLARGE;
    *words = 2ll * nth * M;                                                       // (at most 2^28)
    if (*words > (1ll << 31)) return SLAM2D_E_TOOLARGE;
    return 0;
}

int64_t slam2d_search_points_work(int32_t M, int32_t nx, int32_t ny, int32_t nth) {
    long long words = 0;
    const int rc = check_search_points(M, nx, ny, nth, &words);
    return rc ? rc : words;
}

int slam2d_search_points(const Slam2dLevel* level, int32_t p_field, int32_t nx, int32_t ny, int32_t nth, double x0, double dx, double y0,
                         double dy, double th0, double dth, const double* d_points, int32_t point_stride, int32_t M, uint32_t outside_cost,
                         uint64_t* d_work, uint64_t* d_out, void* stream) {
    const int frc = check_level_field(level, p_field);
    if (frc == SLAM2D_E_BADARG) return frc;
    if (!d_points || !d_out || !d_work || point_stride < 2) return SLAM2D_E_BADARG;
    if (!__builtin_isfinite(dx) || !__builtin_isfinite(dy) || !__builtin_isfinite(dth)) return SLAM2D_E_BADARG;
    long long words = 0;
    const int rc = check_search_points(M, nx, ny, nth, &words);
    if (rc) return rc;
    if (frc) return frc;
    const SearchGrid g = search_grid(nx, ny, nth);
    hipStream_t s = (hipStream_t)stream;
    double2* E = reinterpret_cast<double2*>(d_work);
    k_points_table<<<(unsigned)(g.blocks > nth ? g.blocks : nth), 256, 0, s>>>(nth, th0, dth, d_points, point_stride, M, E, (unsigned long long*)d_out,
                                                                                g.positions);
    k_points_lattice<<<dim3((unsigned)g.blocks, (unsigned)g.rows), 256, 0, s>>>(*level, p_field, nx, g.positions, nth, g.hc, x0, dx, y0, dy, d_points,
                                                                               point_stride, M, E, outside_cost, (unsigned long long*)d_out);
    return launch_status();
}

int slam2d_refine_points(const Slam2dLevel* level, int32_t p_field, int32_t N, const double* d_pose_in, double* d_pose_out, int32_t pose_stride,
                         const double* d_points, int32_t point_stride, int32_t M, int32_t set_stride, const double motion[3], int32_t rx,
                         int32_t ry, int32_t rt, double dx, double dy, double dth, uint32_t outside_cost, uint64_t* d_work, uint64_t* d_out,
                         void* stream) {
    const int frc = check_level_field(level, p_field);
    if (frc == SLAM2D_E_BADARG) return frc;
    if (!d_pose_in || !d_pose_out || !d_points || !d_out || !d_work || d_pose_in == d_pose_out) return SLAM2D_E_BADARG;
    if (N < 1 || pose_stride < 3 || M < 1 || M > SLAM2D_MAX_POINTS || point_stride < 2) return SLAM2D_E_BADARG;
    if (set_stride != 0 && (long long)set_stride < (long long)M * point_stride) return SLAM2D_E_BADARG;
    RefineWindow w;
    const int wrc = check_refine_window(N, M, rx, ry, rt, dx, dy, dth, motion, &w);
    if (wrc) return wrc;
    if (frc) return frc;
    hipStream_t s = (hipStream_t)stream;
    return launch_refine(N, d_pose_in, d_pose_out, pose_stride, motion, w, d_work, d_out, s, [&](unsigned blocks, double* moved, unsigned long long* out) {
        k_refine_points<<<blocks, 256, 0, s>>>(*level, p_field, (int)w.rows, w.hc, w.lat, moved, d_points, point_stride, M, set_stride, outside_cost, out);
    });
}

int64_t slam2d_mcl_work(int32_t N) {
    if (N < 1) return SLAM2D_E_BADARG;
    if (N > SLAM2D_MCL_MAX_PARTICLES) return SLAM2D_E_TOOLARGE;
    return mcl_work_words(N);
}

// What the four MCL steps check alike, for n particles (or that capacity), behind their field check's answer frc; d_source: the
// scan or the point set.  SLAM2D_E_BADARG comes before SLAM2D_E_TOOLARGE -- n first, then the field's --, which a caller returns
// after its own argument checks.
static int check_mcl_particles(int frc, int n, const double* d_pose_in, const double* d_pose_out, int pose_stride, const double* motion,
                               const double* amp, const double* d_source, const uint32_t* d_lut, int lut_n, int lut_shift, const uint64_t* d_work,
                               const uint64_t* d_report) {
    if (frc == SLAM2D_E_BADARG) return frc;
    if (!d_pose_in || !d_pose_out || !motion || !amp || !d_source || !d_lut || !d_work || !d_report) return SLAM2D_E_BADARG;
    if (d_pose_in == d_pose_out || n < 1 || pose_stride < 3 || lut_n < 1 || lut_n > 65536 || lut_shift < 0 || lut_shift > 43)
        return SLAM2D_E_BADARG;
    for (int i = 0; i < 3; ++i)
        if (!__builtin_isfinite(motion[i]) || !__builtin_isfinite(amp[i])) return SLAM2D_E_BADARG;
    return n > SLAM2D_MCL_MAX_PARTICLES ? SLAM2D_E_TOOLARGE : frc;
}
// The scan forms': the lidar's and the level's checks in front
static int check_mcl_step(const Slam2dLidar* lidar, const Slam2dLevel* level, int p_field, int n, const double* d_pose_in, const double* d_pose_out,
                          int pose_stride, const double* motion, const double* amp, const double* d_ranges, const uint32_t* d_lut, int lut_n,
                          int lut_shift, const uint64_t* d_work, const uint64_t* d_report) {
    return check_mcl_particles(check_scored_field(lidar, level, p_field), n, d_pose_in, d_pose_out, pose_stride, motion, amp, d_ranges, d_lut, lut_n,
                               lut_shift, d_work, d_report);
}
// The point forms': the level's checks in front, the set's own (slam2d_refine_points') behind
static int check_mcl_step_points(const Slam2dLevel* level, int p_field, int n, const double* d_pose_in, const double* d_pose_out, int pose_stride,
                                 const double* motion, const double* amp, const double* d_points, int point_stride, int M, const uint32_t* d_lut,
                                 int lut_n, int lut_shift, const uint64_t* d_work, const uint64_t* d_report) {
    const int rc = check_mcl_particles(check_level_field(level, p_field), n, d_pose_in, d_pose_out, pose_stride, motion, amp, d_points, d_lut, lut_n,
                                       lut_shift, d_work, d_report);
    if (rc == SLAM2D_E_BADARG || M < 1 || M > SLAM2D_MAX_POINTS || point_stride < 2) return SLAM2D_E_BADARG;
    return rc;
}

int slam2d_mcl_step(const Slam2dLidar* lidar, const Slam2dLevel* level, int32_t p_field, int32_t N, const double* d_pose_in,
                    double* d_pose_out, int32_t pose_stride, const double motion[3], const double amp[3], uint64_t seed, uint64_t scan,
                    const double* d_ranges, uint32_t outside_cost, const uint32_t* d_lut, int32_t lut_n, int32_t lut_shift,
                    int32_t* d_ancestor, uint64_t* d_work, uint64_t* d_report, void* stream) {
    const int rc = check_mcl_step(lidar, level, p_field, N, d_pose_in, d_pose_out, pose_stride, motion, amp, d_ranges, d_lut, lut_n, lut_shift,
                                  d_work, d_report);
    if (rc) return rc;
    hipStream_t s = (hipStream_t)stream;
    const MclWork wk = mcl_work_of(d_work, N);
    unsigned long long* report = (unsigned long long*)d_report;
    k_mcl_move<<<cdiv(N, 256), 256, 0, s>>>(N, d_pose_in, pose_stride, motion[0], motion[1], motion[2], amp[0], amp[1], amp[2], seed, scan, wk, report);
    k_mcl_score<<<cdiv(N, MCL_WAVES), 64 * MCL_WAVES, 0, s>>>(*lidar, *level, p_field, N, d_ranges, outside_cost, wk);
    k_mcl_weigh<<<cdiv(N, MCL_SCAN_BLOCK), MCL_SCAN_BLOCK / 4, 0, s>>>(N, d_lut, lut_n, lut_shift, wk, report);
    k_mcl_sums<<<1, MCL_SCAN_BLOCK, 0, s>>>(*lidar, N, seed, scan, d_ranges, wk, report);
    k_mcl_resample<<<cdiv(N, 256), 256, 0, s>>>(N, wk, d_pose_out, pose_stride, d_ancestor, report);
    return launch_status();
}

// the checks of the pose bins that slam2d_mcl_step_adaptive and its work size share; *n_bins: nx * ny * nth
static int check_mcl_bins(const Slam2dMclBins* bins, long long* n_bins) {
    if (!bins || bins->nx < 1 || bins->ny < 1 || bins->nth < 1) return SLAM2D_E_BADARG;
    if (!(bins->cell > 0) || !(bins->turn > 0) || !__builtin_isfinite(bins->x0) || !__builtin_isfinite(bins->y0)) return SLAM2D_E_BADARG;
    const long long plane = (long long)bins->nx * bins->ny;                       // (below 2^62; times nth only once it is small)
    if (plane > SLAM2D_MCL_MAX_BINS || plane * bins->nth > SLAM2D_MCL_MAX_BINS) return SLAM2D_E_TOOLARGE;
    *n_bins = plane * bins->nth;
    return 0;
}

int64_t slam2d_mcl_adapt_work(int32_t n_cap, const Slam2dMclBins* bins) {
    long long n_bins = 0;
    const int rc = check_mcl_bins(bins, &n_bins);
    if (rc == SLAM2D_E_BADARG || n_cap < 1) return SLAM2D_E_BADARG;
    if (n_cap > SLAM2D_MCL_MAX_PARTICLES) return SLAM2D_E_TOOLARGE;
    if (rc) return rc;
    return mcl_work_words(n_cap) + mcla_bitmap_words(n_bins) + MCLA_TAIL;
}

// What the two adaptive steps check behind their plain step's answer rc; *n_bins: nx * ny * nth
static int check_mcl_adaptive(int rc, const uint32_t* d_n_in, const uint32_t* d_n_out, const uint32_t* d_ntab, int ntab_n, const Slam2dMclBins* bins,
                              long long* n_bins) {
    if (rc == SLAM2D_E_BADARG) return rc;
    if (!d_n_in || !d_n_out || !d_ntab || ntab_n < 1 || ntab_n > 65536) return SLAM2D_E_BADARG;
    const int brc = check_mcl_bins(bins, n_bins);
    if (brc == SLAM2D_E_BADARG) return brc;
    return rc ? rc : brc;
}
// d_work of an adaptive step and the grids of its launches over the capacity: slam2d_mcl_step's arrays, the bitmap, the tail
struct MclaWork { MclWork wk; unsigned long long *bitmap, *tail; int words, per_particle, move_blocks, score_blocks; };
static MclaWork mcla_work_of(uint64_t* d_work, int n_cap, long long n_bins) {
    const int words = (int)mcla_bitmap_words(n_bins);                             // (at most 2^20 + 1)
    unsigned long long* bitmap = (unsigned long long*)d_work + mcl_work_words(n_cap);
    return MclaWork{mcl_work_of(d_work, n_cap), bitmap, bitmap + words, words, min(cdiv(n_cap, 256), MCLA_BLOCKS),
                    min(max(cdiv(n_cap, 256), cdiv(words, 256)), MCLA_BLOCKS), min(cdiv(n_cap, MCL_WAVES), MCLA_SCORE_BLOCKS)};
}
// The last three launches of an adaptive step: the reference ancestors and their bins, the bitmap's count, the resampling
static int launch_mcla_resampling(const MclaWork& a, int n_cap, const uint32_t* d_n_in, uint32_t* d_n_out, const Slam2dMclBins& bins,
                                  const uint32_t* d_ntab, int ntab_n, double* d_pose_out, int pose_stride, int32_t* d_ancestor,
                                  unsigned long long* report, hipStream_t s) {
    k_mcla_refs<<<min(a.per_particle, MCLA_REF_BLOCKS), 256, 0, s>>>(d_n_in, n_cap, a.wk, bins, a.bitmap, a.tail, report);
    k_mcla_count<<<min(cdiv(a.words, 256), MCLA_BLOCKS), 256, 0, s>>>(a.bitmap, a.words, a.tail);
    k_mcla_resample<<<a.per_particle, 256, 0, s>>>(n_cap, d_ntab, ntab_n, a.wk, a.tail, d_pose_out, pose_stride, d_ancestor, d_n_out, report);
    return launch_status();
}

int slam2d_mcl_step_adaptive(const Slam2dLidar* lidar, const Slam2dLevel* level, int32_t p_field, int32_t n_cap, const uint32_t* d_n_in,
                             uint32_t* d_n_out, const double* d_pose_in, double* d_pose_out, int32_t pose_stride, const double motion[3],
                             const double amp[3], uint64_t seed, uint64_t scan, const double* d_ranges, uint32_t outside_cost,
                             const uint32_t* d_lut, int32_t lut_n, int32_t lut_shift, const Slam2dMclBins* bins, const uint32_t* d_ntab,
                             int32_t ntab_n, int32_t* d_ancestor, uint64_t* d_work, uint64_t* d_report, void* stream) {
    long long n_bins = 0;
    const int rc = check_mcl_adaptive(check_mcl_step(lidar, level, p_field, n_cap, d_pose_in, d_pose_out, pose_stride, motion, amp, d_ranges, d_lut,
                                                     lut_n, lut_shift, d_work, d_report), d_n_in, d_n_out, d_ntab, ntab_n, bins, &n_bins);
    if (rc) return rc;
    hipStream_t s = (hipStream_t)stream;
    const MclaWork a = mcla_work_of(d_work, n_cap, n_bins);
    unsigned long long* report = (unsigned long long*)d_report;
    k_mcla_move<<<a.move_blocks, 256, 0, s>>>(d_n_in, n_cap, d_pose_in, pose_stride, motion[0], motion[1], motion[2], amp[0], amp[1], amp[2], seed, scan,
                                              a.wk, a.bitmap, a.words, a.tail, report);
    k_mcla_score<<<a.score_blocks, 64 * MCL_WAVES, 0, s>>>(*lidar, *level, p_field, d_n_in, n_cap, d_ranges, outside_cost, a.wk);
    k_mcla_weigh<<<cdiv(n_cap, MCL_SCAN_BLOCK), MCL_SCAN_BLOCK / 4, 0, s>>>(d_n_in, n_cap, d_lut, lut_n, lut_shift, a.wk, report);
    k_mcla_sums<<<1, MCL_SCAN_BLOCK, 0, s>>>(*lidar, d_n_in, n_cap, seed, scan, d_ranges, a.wk, report);
    return launch_mcla_resampling(a, n_cap, d_n_in, d_n_out, *bins, d_ntab, ntab_n, d_pose_out, pose_stride, d_ancestor, report, s);
}

int64_t slam2d_mcl_rays_work(int32_t N) { return slam2d_mcl_work(N); }
int64_t slam2d_mcl_adapt_rays_work(int32_t n_cap, const Slam2dMclBins* bins) { return slam2d_mcl_adapt_work(n_cap, bins); }

// What the two ray steps check behind their plain step's answer rc: SLAM2D_E_BADARG in front of its SLAM2D_E_TOOLARGE
static int check_mcl_rays(int rc, const uint32_t* d_dist2, int ray_stride, int ray_phase, int margin) {
    if (rc == SLAM2D_E_BADARG) return rc;
    if (!d_dist2 || ray_stride < 1 || ray_stride > SLAM2D_MAX_BEAMS || ray_phase < 0 || ray_phase >= ray_stride || margin < 0) return SLAM2D_E_BADARG;
    return rc;
}

int slam2d_mcl_step_rays(const Slam2dLidar* lidar, const Slam2dLevel* level, int32_t p_field, const uint32_t* d_dist2, int32_t N,
                         const double* d_pose_in, double* d_pose_out, int32_t pose_stride, const double motion[3], const double amp[3],
                         uint64_t seed, uint64_t scan, const double* d_ranges, uint32_t outside_cost, int32_t ray_stride, int32_t ray_phase,
                         int32_t margin, uint32_t through_cost, const uint32_t* d_lut, int32_t lut_n, int32_t lut_shift, int32_t* d_ancestor,
                         uint32_t* d_through, uint64_t* d_work, uint64_t* d_report, void* stream) {
    const int rc = check_mcl_rays(check_mcl_step(lidar, level, p_field, N, d_pose_in, d_pose_out, pose_stride, motion, amp, d_ranges, d_lut, lut_n,
                                                 lut_shift, d_work, d_report), d_dist2, ray_stride, ray_phase, margin);
    if (rc) return rc;
    hipStream_t s = (hipStream_t)stream;
    const MclWork wk = mcl_work_of(d_work, N);
    const MclRays ry{ray_stride, ray_phase, margin, through_cost, d_through};
    unsigned long long* report = (unsigned long long*)d_report;
    k_mcl_move_rays<<<cdiv(N, 256), 256, 0, s>>>(N, d_pose_in, pose_stride, motion[0], motion[1], motion[2], amp[0], amp[1], amp[2], seed, scan, wk, report);
    k_mcl_score_rays<<<cdiv(N, MCLR_WAVES), 64 * MCLR_WAVES, 0, s>>>(*lidar, *level, p_field, d_dist2, N, d_ranges, outside_cost, ry, wk, report);
    k_mcl_weigh<<<cdiv(N, MCL_SCAN_BLOCK), MCL_SCAN_BLOCK / 4, 0, s>>>(N, d_lut, lut_n, lut_shift, wk, report);
    k_mcl_sums_rays<<<1, MCL_SCAN_BLOCK, 0, s>>>(*lidar, N, seed, scan, d_ranges, wk, report);
    k_mcl_resample<<<cdiv(N, 256), 256, 0, s>>>(N, wk, d_pose_out, pose_stride, d_ancestor, report);
    return launch_status();
}

int slam2d_mcl_step_adaptive_rays(const Slam2dLidar* lidar, const Slam2dLevel* level, int32_t p_field, const uint32_t* d_dist2, int32_t n_cap,
                                  const uint32_t* d_n_in, uint32_t* d_n_out, const double* d_pose_in, double* d_pose_out, int32_t pose_stride,
                                  const double motion[3], const double amp[3], uint64_t seed, uint64_t scan, const double* d_ranges,
                                  uint32_t outside_cost, int32_t ray_stride, int32_t ray_phase, int32_t margin, uint32_t through_cost,
                                  const uint32_t* d_lut, int32_t lut_n, int32_t lut_shift, const Slam2dMclBins* bins, const uint32_t* d_ntab,
                                  int32_t ntab_n, int32_t* d_ancestor, uint32_t* d_through, uint64_t* d_work, uint64_t* d_report, void* stream) {
    long long n_bins = 0;
    const int rc = check_mcl_adaptive(check_mcl_rays(check_mcl_step(lidar, level, p_field, n_cap, d_pose_in, d_pose_out, pose_stride, motion, amp,
                                                                    d_ranges, d_lut, lut_n, lut_shift, d_work, d_report),
                                                     d_dist2, ray_stride, ray_phase, margin), d_n_in, d_n_out, d_ntab, ntab_n, bins, &n_bins);
    if (rc) return rc;
    hipStream_t s = (hipStream_t)stream;
    const MclaWork a = mcla_work_of(d_work, n_cap, n_bins);
    const MclRays ry{ray_stride, ray_phase, margin, through_cost, d_through};
    unsigned long long* report = (unsigned long long*)d_report;
    k_mcla_move_rays<<<a.move_blocks, 256, 0, s>>>(d_n_in, n_cap, d_pose_in, pose_stride, motion[0], motion[1], motion[2], amp[0], amp[1], amp[2], seed,
                                                   scan, a.wk, a.bitmap, a.words, a.tail, report);
    k_mcla_score_rays<<<cdiv(a.score_blocks * MCL_WAVES, MCLR_WAVES), 64 * MCLR_WAVES, 0, s>>>(*lidar, *level, p_field, d_dist2, d_n_in, n_cap, d_ranges, outside_cost, ry, a.wk, report);
    k_mcla_weigh<<<cdiv(n_cap, MCL_SCAN_BLOCK), MCL_SCAN_BLOCK / 4, 0, s>>>(d_n_in, n_cap, d_lut, lut_n, lut_shift, a.wk, report);
    k_mcla_sums_rays<<<1, MCL_SCAN_BLOCK, 0, s>>>(*lidar, d_n_in, n_cap, seed, scan, d_ranges, a.wk, report);
    return launch_mcla_resampling(a, n_cap, d_n_in, d_n_out, *bins, d_ntab, ntab_n, d_pose_out, pose_stride, d_ancestor, report, s);
}

int64_t slam2d_mcl_points_work(int32_t N) {
    const int64_t words = slam2d_mcl_work(N);
    return words < 0 ? words : words + 2ll * N;                                   // behind the scan form's: cos / sin of the moved headings
}

int slam2d_mcl_step_points(const Slam2dLevel* level, int32_t p_field, int32_t N, const double* d_pose_in, double* d_pose_out, int32_t pose_stride,
                           const double motion[3], const double amp[3], uint64_t seed, uint64_t scan, const double* d_points,
                           int32_t point_stride, int32_t M, uint32_t outside_cost, const uint32_t* d_lut, int32_t lut_n, int32_t lut_shift,
                           int32_t* d_ancestor, uint64_t* d_work, uint64_t* d_report, void* stream) {
    const int rc = check_mcl_step_points(level, p_field, N, d_pose_in, d_pose_out, pose_stride, motion, amp, d_points, point_stride, M, d_lut, lut_n,
                                         lut_shift, d_work, d_report);
    if (rc) return rc;
    hipStream_t s = (hipStream_t)stream;
    const MclWork wk = mcl_work_of(d_work, N);
    double* cs = reinterpret_cast<double*>(d_work + mcl_work_words(N));
    unsigned long long* report = (unsigned long long*)d_report;
    k_mclp_move<<<cdiv(N, 256), 256, 0, s>>>(N, d_pose_in, pose_stride, motion[0], motion[1], motion[2], amp[0], amp[1], amp[2], seed, scan, wk, cs, report);
    k_mclp_score<<<cdiv(N, MCLP_WAVES), 64 * MCLP_WAVES, 0, s>>>(*level, p_field, N, d_points, point_stride, M, outside_cost, wk, cs);
    k_mcl_weigh<<<cdiv(N, MCL_SCAN_BLOCK), MCL_SCAN_BLOCK / 4, 0, s>>>(N, d_lut, lut_n, lut_shift, wk, report);
    k_mclp_sums<<<1, MCL_SCAN_BLOCK, 0, s>>>(N, seed, scan, d_points, point_stride, M, wk, report);
    k_mcl_resample<<<cdiv(N, 256), 256, 0, s>>>(N, wk, d_pose_out, pose_stride, d_ancestor, report);
    return launch_status();
}

int64_t slam2d_mcl_adapt_points_work(int32_t n_cap, const Slam2dMclBins* bins) {
    const int64_t words = slam2d_mcl_adapt_work(n_cap, bins);
    return words < 0 ? words : words + 2ll * n_cap;                               // behind the scan form's, as in slam2d_mcl_points_work
}

int slam2d_mcl_step_adaptive_points(const Slam2dLevel* level, int32_t p_field, int32_t n_cap, const uint32_t* d_n_in, uint32_t* d_n_out,
                                    const double* d_pose_in, double* d_pose_out, int32_t pose_stride, const double motion[3], const double amp[3],
                                    uint64_t seed, uint64_t scan, const double* d_points, int32_t point_stride, int32_t M, uint32_t outside_cost,
                                    const uint32_t* d_lut, int32_t lut_n, int32_t lut_shift, const Slam2dMclBins* bins, const uint32_t* d_ntab,
                                    int32_t ntab_n, int32_t* d_ancestor, uint64_t* d_work, uint64_t* d_report, void* stream) {
    long long n_bins = 0;
    const int rc = check_mcl_adaptive(check_mcl_step_points(level, p_field, n_cap, d_pose_in, d_pose_out, pose_stride, motion, amp, d_points,
                                                            point_stride, M, d_lut, lut_n, lut_shift, d_work, d_report),
                                      d_n_in, d_n_out, d_ntab, ntab_n, bins, &n_bins);
    if (rc) return rc;
    hipStream_t s = (hipStream_t)stream;
    const MclaWork a = mcla_work_of(d_work, n_cap, n_bins);
    double* cs = reinterpret_cast<double*>(a.tail + MCLA_TAIL);
    unsigned long long* report = (unsigned long long*)d_report;
    k_mclap_move<<<a.move_blocks, 256, 0, s>>>(d_n_in, n_cap, d_pose_in, pose_stride, motion[0], motion[1], motion[2], amp[0], amp[1], amp[2], seed, scan,
                                               a.wk, cs, a.bitmap, a.words, a.tail, report);
    k_mclap_score<<<cdiv(a.score_blocks * MCL_WAVES, MCLP_WAVES), 64 * MCLP_WAVES, 0, s>>>(*level, p_field, d_n_in, n_cap, d_points, point_stride, M, outside_cost, a.wk, cs);
    k_mcla_weigh<<<cdiv(n_cap, MCL_SCAN_BLOCK), MCL_SCAN_BLOCK / 4, 0, s>>>(d_n_in, n_cap, d_lut, lut_n, lut_shift, a.wk, report);
    k_mclap_sums<<<1, MCL_SCAN_BLOCK, 0, s>>>(d_n_in, n_cap, seed, scan, d_points, point_stride, M, a.wk, report);
    return launch_mcla_resampling(a, n_cap, d_n_in, d_n_out, *bins, d_ntab, ntab_n, d_pose_out, pose_stride, d_ancestor, report, s);
}

int slam2d_grid_update_weights(const Slam2dLidar* lidar, const Slam2dMap* d_maps, int32_t P, const double* d_pose,
                               int32_t pose_stride, const double* d_ranges, uint32_t* d_flags, double* d_logw,
                               const double* d_logconf, int32_t logconf_stride, double* d_w, double* d_stats, void* stream) {
    if (!d_logw || !d_w || !d_stats || (d_logconf && logconf_stride < 1)) return SLAM2D_E_BADARG;
    return launch_update(lidar, d_maps, P, d_pose, pose_stride, d_ranges, nullptr, d_flags,
                         WeightsJob{d_logw, d_logconf, logconf_stride, P, d_w, d_stats, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr}, stream);
}

int slam2d_grid_update_weights_local(const Slam2dLidar* lidar, const Slam2dMap* d_maps, int32_t P, const double* d_pose,
                                     int32_t pose_stride, const double* d_ranges, uint32_t* d_flags, double* d_logw,
                                     const double* d_logconf, int32_t logconf_stride, double* d_part, void* stream) {
    if (!d_logw || !d_part || (d_logconf && logconf_stride < 1)) return SLAM2D_E_BADARG;
    return launch_update(lidar, d_maps, P, d_pose, pose_stride, d_ranges, nullptr, d_flags,
                         WeightsJob{d_logw, d_logconf, logconf_stride, P, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr,
                                    nullptr, d_part}, stream);
}

int slam2d_prior(const double* d_prev_pose, double raw_theta, double prev_raw_theta, int32_t has_turn,
                 double raw_turn, const double* d_heading, int32_t P, double* d_est, double* d_psi_cs,
                 void* stream) {
    if (!d_prev_pose || !d_heading || !d_est || !d_psi_cs || P <= 0) return SLAM2D_E_BADARG;
    k_prior<<<cdiv(P, 64), 64, 0, (hipStream_t)stream>>>(d_prev_pose, raw_theta, prev_raw_theta, has_turn, raw_turn,
                                                         d_heading, P, d_est, d_psi_cs);
    return launch_status();
}

int slam2d_post_match(const Slam2dMatch* d_fine, const Slam2dMatch* d_coarse, int32_t P, double* d_prev_pose,
                      double* d_heading, double* d_logw, double* d_report, void* stream) {
    if (!d_fine || !d_coarse || !d_prev_pose || !d_heading || !d_logw || P <= 0) return SLAM2D_E_BADARG;
    k_post_match<<<cdiv(P, 64), 64, 0, (hipStream_t)stream>>>(d_fine, d_coarse, P, d_prev_pose, d_heading, d_logw, d_report);
    return launch_status();
}

int slam2d_weights_normalize(double* d_logw, const double* d_logconf, int32_t logconf_stride, int32_t N, double* d_w,
                             double* d_stats, void* stream) {
    if (!d_logw || !d_w || !d_stats || N <= 0 || (d_logconf && logconf_stride < 1)) return SLAM2D_E_BADARG;
    k_weights<<<1, 256, 0, (hipStream_t)stream>>>(d_logw, d_logconf, logconf_stride, N, d_w, d_stats, nullptr, nullptr);
    return launch_status();
}

int slam2d_scan_match(const Slam2dLidar* lidar, const Slam2dLevel* coarse, const Slam2dLevel* fine, const Slam2dMap* d_maps,
                      int32_t P, const double* d_prev_pose, double raw_theta, double prev_raw_theta, int32_t has_turn,
                      double raw_turn, const double* d_heading, const double* d_ranges, double est_moving_dist,
                      const double* d_uniform, double* d_est, double* d_psi_cs, Slam2dMatch* d_coarse, Slam2dMatch* d_fine,
                      uint32_t* d_flags, uint32_t options, void* stream) {
    // (SLAM2D_MATCH_PRIOR_READY: d_est / d_psi_cs were written by the previous scan's slam2d_scan_commit_next)
    int rc = (options & SLAM2D_MATCH_PRIOR_READY) ? 0
             : slam2d_prior(d_prev_pose, raw_theta, prev_raw_theta, has_turn, raw_turn, d_heading, P, d_est, d_psi_cs, stream);
    if (rc) return rc;
    rc = slam2d_match(lidar, coarse, d_maps, P, d_est, 3, d_ranges, est_moving_dist, d_psi_cs, d_uniform, d_coarse, d_flags,
                      options & ~SLAM2D_MATCH_PRIOR_READY, stream);
    if (rc) return rc;
    // the fine level is centred on the coarse result and takes its arg-max (matchMax=True), priors off (:65-73)
    return slam2d_match(lidar, fine, d_maps, P, reinterpret_cast<const double*>(d_coarse), (int32_t)(sizeof(Slam2dMatch) / sizeof(double)),
                        d_ranges, est_moving_dist, nullptr, nullptr, d_fine, d_flags, 0u, stream);
}

int slam2d_scan_commit(const Slam2dLidar* lidar, const Slam2dMap* d_maps, int32_t P, const Slam2dMatch* d_fine,
                       const Slam2dMatch* d_coarse, double* d_prev_pose, double* d_heading, double* d_logw, double* d_report,
                       const double* d_ranges, uint32_t* d_flags, double* d_w, double* d_stats, uint32_t* d_flag_snapshot,
                       uint32_t abort_mask, void* stream) {
    return slam2d_scan_commit_next(lidar, d_maps, P, d_fine, d_coarse, d_prev_pose, d_heading, d_logw, d_report, d_ranges, d_flags, d_w,
                                   d_stats, d_flag_snapshot, abort_mask, 0.0, 0.0, 0, 0.0, nullptr, nullptr, stream);
}

int slam2d_scan_commit_next(const Slam2dLidar* lidar, const Slam2dMap* d_maps, int32_t P, const Slam2dMatch* d_fine,
                            const Slam2dMatch* d_coarse, double* d_prev_pose, double* d_heading, double* d_logw, double* d_report,
                            const double* d_ranges, uint32_t* d_flags, double* d_w, double* d_stats, uint32_t* d_flag_snapshot,
                            uint32_t abort_mask, double next_raw_theta, double next_prev_raw_theta, int32_t next_has_turn,
                            double next_raw_turn, double* d_next_est, double* d_next_psi_cs, void* stream) {
    if ((d_next_est != nullptr) != (d_next_psi_cs != nullptr) || (d_next_est && !d_w)) return SLAM2D_E_BADARG;
    if (!d_w) {                                        // sharded filters run their own normaliser (a collective sits in it)
        const int rc = slam2d_post_match(d_fine, d_coarse, P, d_prev_pose, d_heading, d_logw, d_report, stream);
        if (rc) return rc;
        return slam2d_grid_update(lidar, d_maps, P, d_prev_pose, 3, d_ranges, nullptr, d_flags, stream);
    }
    if (!d_fine || !d_coarse || !d_prev_pose || !d_heading || !d_logw || !d_stats || !d_flag_snapshot) return SLAM2D_E_BADARG;
    // ONE launch: the update blocks read the matched poses from d_fine; one extra block does the bookkeeping
    // (k_post_match's work) and then the normaliser, which needs nothing the update writes
    static_assert(sizeof(Slam2dMatch) % sizeof(double) == 0, "Slam2dMatch is read as rows of doubles");
    return launch_update(lidar, d_maps, P, reinterpret_cast<const double*>(d_fine), (int)(sizeof(Slam2dMatch) / sizeof(double)), d_ranges,
                         nullptr, d_flags,
                         WeightsJob{d_logw, nullptr, 1, P, d_w, d_stats, d_flags, d_flag_snapshot, d_fine, d_coarse, d_prev_pose, d_heading,
                                    d_report, nullptr, abort_mask, nullptr, 0, d_next_est, d_next_psi_cs, next_raw_theta,
                                    next_prev_raw_theta, next_raw_turn, next_has_turn}, stream);
}

// ---- particle groups on several streams, one host call per scan (include/slam2d.h, "one scan for several particle GROUPS") ----
// The normaliser merged by the groups' own blocks (Slam2dScan.d_norm_sync): one rank (the sharded merge has an all-gather in front of
// it), no abort decision across groups (a voided scan's groups would not all arrive), the groups' partials in d_parts in group order.
// (round 5, ABI 16: ... or an abort decided behind k_match_arrive / k_abort_gate, Slam2dScan.match_seq != 0)
#define SLAM2D_SYNC_MAX_GROUPS 56       // words 2 .. 57 of the sync block: one per group; 59: the waits' bound; 60-62: tickets and flags
static inline bool abort_on_device(const Slam2dScan& sc) { return sc.d_norm_sync != nullptr && sc.match_seq != 0u; }
static inline bool device_merged(const Slam2dScan& sc) { return sc.d_norm_sync != nullptr && sc.merge && (!sc.abort_mask || sc.match_seq != 0u); }
// ... or only synchronised through those words (merge == 0, the sharded normaliser: slam2d_norm_gate, the collective and
// slam2d_weights_merge_publish follow on the caller's stream)
static inline bool device_synced(const Slam2dScan& sc) { return sc.d_norm_sync != nullptr && (!sc.abort_mask || sc.match_seq != 0u); }
static int groups_check(const Slam2dLidar* lidar, const Slam2dGroup* groups, int32_t G, const Slam2dScan* sc, bool commit) {
    if (!lidar || !groups || !sc || G <= 0 || G > 64 || (!sc->d_ranges && !sc->h_ranges)) return SLAM2D_E_BADARG;
    if (sc->match_seq && !sc->d_norm_sync) return SLAM2D_E_BADARG;
    if (sc->h_seq && (!device_merged(*sc) || !sc->h_pack || !sc->d_pack || sc->pack_doubles <= 0)) return SLAM2D_E_BADARG;
    for (int i = 0; i < G; ++i) {
        const Slam2dGroup& g = groups[i];
        if (!g.coarse || !g.d_maps || g.P <= 0 || !g.d_coarse || (g.fine && !g.d_fine) || !g.d_flags || (!g.ev_done && !sc->d_norm_sync)) return SLAM2D_E_BADARG;
        if (g.d_est ? g.est_stride < 3 : (!g.d_prev_pose || !g.d_heading || !g.d_est_out || !g.d_psi_out)) return SLAM2D_E_BADARG;
        if (commit && (!g.d_logw || !g.d_part)) return SLAM2D_E_BADARG;
        if (commit && sc->abort_mask && !g.ev_matched && !abort_on_device(*sc)) return SLAM2D_E_BADARG;
        if (sc->h_ranges && (g.d_est || !g.d_pull)) return SLAM2D_E_BADARG;          // (the pull rides in the closed loop's prior launch)
        if (commit && sc->h_next_ranges && (!sc->h_ranges || !g.d_pull_next || !device_synced(*sc))) return SLAM2D_E_BADARG;
    }
    if (commit) {
        const bool dm = device_merged(*sc);
        if (!dm && !sc->norm_stream && sc->merge) return SLAM2D_E_BADARG;
        if (sc->merge && (!sc->d_logw_all || !sc->d_parts || !sc->d_w || !sc->d_stats || (!dm && !sc->ev_merged) || sc->n_local <= 0 || sc->n_parts <= 0 ||
                          sc->total_particles < sc->n_local)) return SLAM2D_E_BADARG;
        if (dm && sc->n_parts != G) return SLAM2D_E_BADARG;                  // (one partial per group, in group order)
        if (sc->d_norm_sync && (G > SLAM2D_SYNC_MAX_GROUPS || (sc->abort_mask && !sc->match_seq))) return SLAM2D_E_BADARG;  // (2 + G words, 59-62 taken; an abort
        //                                                             decision across groups needs the events or k_match_arrive / k_abort_gate)
        if (sc->abort_mask && (!sc->d_abort_flags || sc->n_abort_flags <= 0)) return SLAM2D_E_BADARG;
    }
    return 0;
}

static int group_match(const Slam2dLidar* lidar, const Slam2dGroup& g, const Slam2dScan& sc, const int G, const bool step = false) {
    hipStream_t s = (hipStream_t)g.stream;
    int rc = 0;
    if (sc.ev_inputs && (rc = (int)hipStreamWaitEvent(s, (hipEvent_t)sc.ev_inputs, 0))) return rc;
    const double* est = g.d_est;
    const double* psi = g.d_psi_cs;
    int stride = g.est_stride;
    const double* ranges = sc.d_ranges;
    const double* uniform = g.d_uniform;
    if (!est) {                                        // closed loop: the pose prior from the previous matched poses
        if (sc.h_ranges) {                             // ... and the scan's ranges pulled from pinned host memory in the same launch
            if (!(sc.options & SLAM2D_MATCH_PRIOR_READY)) {             // (else: the previous commit did both, Slam2dScan.h_next_ranges)
                k_prior_pull<<<1, 256, 0, s>>>(g.d_prev_pose, sc.raw_theta, sc.prev_raw_theta, sc.has_turn, sc.raw_turn, g.d_heading, g.P,
                                               g.d_est_out, g.d_psi_out, sc.h_ranges, lidar->beams, g.d_pull);
                if ((rc = launch_status())) return rc;
            }
            ranges = g.d_pull; uniform = g.h_uniform;
        } else if ((rc = slam2d_prior(g.d_prev_pose, sc.raw_theta, sc.prev_raw_theta, sc.has_turn, sc.raw_turn, g.d_heading, g.P, g.d_est_out,
                                      g.d_psi_out, g.stream))) return rc;
        est = g.d_est_out; psi = g.d_psi_out; stride = 3;
    }
    if ((rc = slam2d_match(lidar, g.coarse, g.d_maps, g.P, est, stride, ranges, sc.est_moving_dist, psi, uniform, g.d_coarse,
                           g.d_flags, sc.options & ~SLAM2D_MATCH_PRIOR_READY, g.stream))) return rc;
    const bool count_in = abort_on_device(sc) && !step && G > 1;       // (one group: its stream orders its commit behind its match)
    if (g.fine) {
        Slam2dLevel last = *g.fine;                    // (the level whose selecting waves count their particles in for the commit's gate)
        if (count_in) last.arrive = sc.d_norm_sync + 61;
        if ((rc = slam2d_match(lidar, &last, g.d_maps, g.P, reinterpret_cast<const double*>(g.d_coarse),
                               (int32_t)(sizeof(Slam2dMatch) / sizeof(double)), ranges, sc.est_moving_dist, nullptr, nullptr,
                               g.d_fine, g.d_flags, 0u, g.stream))) return rc;
    } else if (count_in) {
        k_match_arrive<<<1, 64, 0, s>>>(sc.d_norm_sync, (uint32_t)g.P);
        if ((rc = launch_status())) return rc;
    }
    if (abort_on_device(sc) && !step) return rc;
    // (ev_matched serves a LATER commit call's abort decision; slam2d_groups_step has none, and an event packet between two kernels
    // of a group costs its chain 3 us)
    if (g.ev_matched && !step) rc = (int)hipEventRecord((hipEvent_t)g.ev_matched, s);
    return rc;
}

static int group_commit(const Slam2dLidar* lidar, const Slam2dGroup* groups, int32_t G, int i, const Slam2dScan& sc) {
    const Slam2dGroup& g = groups[i];
    hipStream_t s = (hipStream_t)g.stream;
    int rc = 0;
    if (sc.abort_mask && abort_on_device(sc)) {        // the abort is decided over every group's fault bits: wait for every group's match
        if (G > 1) {
            k_abort_gate<<<1, 64, 0, s>>>(sc.d_norm_sync, (uint32_t)sc.n_abort_flags * sc.match_seq, g.d_flags);
            if ((rc = launch_status())) return rc;
        }
    } else if (sc.abort_mask)
        for (int j = 0; j < G; ++j)
            if (j != i && (rc = (int)hipStreamWaitEvent(s, (hipEvent_t)groups[j].ev_matched, 0))) return rc;
    // the previous scan's merge works on the log-weights this launch rewrites: an event behind the merge launch -- or, with
    // Slam2dScan.d_norm_sync, nothing on the stream: the normaliser blocks settle it on the device (normaliser_wait / _arrive)
    const bool device_merge = device_merged(sc), device_sync = device_synced(sc);
    if (!device_sync && sc.wait_merged && sc.ev_merged && (rc = (int)hipStreamWaitEvent(s, (hipEvent_t)sc.ev_merged, 0))) return rc;
    const Slam2dMatch* fin = g.fine ? g.d_fine : g.d_coarse;
    const int md = (int)(sizeof(Slam2dMatch) / sizeof(double));
    WeightsJob wj = g.d_est                            // open loop: weight *= coarse confidence, update at the matched pose
        ? WeightsJob{g.d_logw, &g.d_coarse->log_confidence, md, g.P, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr,
                     nullptr, nullptr, g.d_part, 0u, nullptr, 0}
        // closed loop: slam2d_scan_commit's launch with the normaliser's local half
        : WeightsJob{g.d_logw, nullptr, 1, g.P, nullptr, nullptr, g.d_flags, g.d_flag_snapshot, fin, g.d_coarse, g.d_prev_pose,
                     g.d_heading, g.d_report, g.d_part, sc.abort_mask, sc.d_abort_flags, sc.n_abort_flags};
    if (device_sync) { wj.nsync = sc.d_norm_sync; wj.ngroups = G; wj.gidx = i; }
    if (device_merge) {
        wj.parts_all = sc.d_parts; wj.logw_all = sc.d_logw_all; wj.n_all = sc.n_local; wj.total = (double)sc.total_particles;
        wj.w_all = sc.d_w; wj.stats_all = sc.d_stats;
        if (sc.h_seq) { wj.pack_d = sc.d_pack; wj.pack_h = sc.h_pack; wj.pack_n = sc.pack_doubles; wj.h_seq = sc.h_seq; wj.seq = sc.report_seq; }
    }
    if (device_sync && sc.h_next_ranges && !g.d_est) {  // closed loop: the next scan's prior and ranges ride in this launch's block 0 (needs the
        //                                                 matched poses only: a sharded rank's commit, which does not merge, carries them too)
        wj.next_est = g.d_est_out; wj.next_psi = g.d_psi_out; wj.next_raw_theta = sc.next_raw_theta;
        wj.next_prev_raw_theta = sc.next_prev_raw_theta; wj.next_raw_turn = sc.next_raw_turn; wj.next_has_turn = sc.next_has_turn;
        wj.pull_src = sc.h_next_ranges; wj.pull_dst = g.d_pull_next; wj.pull_n = lidar->beams;
    }
    rc = launch_update(lidar, g.d_maps, g.P, reinterpret_cast<const double*>(fin), md, sc.h_ranges ? g.d_pull : sc.d_ranges, nullptr, g.d_flags, wj, g.stream);
    if (rc || (device_sync && !g.ev_done)) return rc;
    return (int)hipEventRecord((hipEvent_t)g.ev_done, s);
}

static int groups_merge(const Slam2dGroup* groups, int32_t G, const Slam2dScan& sc) {
    if (device_merged(sc)) return 0;                   // the last group's normaliser block has merged (or will)
    if (device_synced(sc)) return 0;                   // (merge == 0: the caller's slam2d_norm_gate orders its stream behind the groups)
    hipStream_t ns = (hipStream_t)sc.norm_stream;
    int rc = 0;
    for (int i = 0; i < G; ++i)
        if ((rc = (int)hipStreamWaitEvent(ns, (hipEvent_t)groups[i].ev_done, 0))) return rc;
    if (!sc.merge) return 0;                           // sharded: the caller's all-gather and slam2d_weights_merge follow on norm_stream
    k_weights_merge<<<1, 256, 0, ns>>>(sc.d_logw_all, sc.n_local, sc.d_parts, sc.n_parts, (double)sc.total_particles, sc.d_w, sc.d_stats,
                                       sc.d_abort_flags, sc.n_abort_flags, sc.d_abort_flags ? sc.abort_mask : 0u);
    if ((rc = launch_status())) return rc;
    return (int)hipEventRecord((hipEvent_t)sc.ev_merged, ns);
}

// One host thread per group beyond the first: a HIP launch costs the calling thread ~4-5 us, a group's scan 7-15 launches, so
// issuing G groups from one thread takes G x 35-70 us -- as long as the device needs for the whole scan from two groups up
// (round 4: 0.076-0.109 ms of a 0.133 ms step with two groups, host-bound with four; the closed loop, twice the launches per
// scan, ran SLOWER in two groups than in one).  The workers spin briefly between scans (a condition variable's wake-up costs as
// much as the job) and sleep when no scan has come for a while.  SLAM2D_GROUP_THREADS=0: everything from the calling thread.
enum { JOB_MATCH = 1, JOB_COMMIT = 2, JOB_STEP = 3 };
static int run_group_job(int kind, const Slam2dLidar* lidar, const Slam2dGroup* groups, int G, int i, const Slam2dScan& sc) {
    int rc = 0;
    if (kind & JOB_MATCH) rc = group_match(lidar, groups[i], sc, G, kind == JOB_STEP);
    if (!rc && (kind & JOB_COMMIT)) rc = group_commit(lidar, groups, G, i, sc);
    return rc;
}
// Host cores this process may really use: the scheduler affinity capped by the cgroup CPU quota (v2 cpu.max, v1 cfs quota) --
// what bench.effective_cores() reports.  A container often sees every core of the host and may use a few.
static int effective_cores() {
    int n = (int)std::thread::hardware_concurrency();
    if (n < 1) n = 1;
    cpu_set_t set;
    CPU_ZERO(&set);
    if (sched_getaffinity(0, sizeof(set), &set) == 0) { const int c = CPU_COUNT(&set); if (c >= 1 && c < n) n = c; }
    if (FILE* f = fopen("/sys/fs/cgroup/cpu.max", "r")) {
        char q[64] = {0}; double period = 0.0;
        if (fscanf(f, "%63s %lf", q, &period) == 2 && strcmp(q, "max") != 0 && period > 0.0) { const int c = (int)(atof(q) / period); if (c < n) n = c < 1 ? 1 : c; }
        fclose(f);
    } else if (FILE* g = fopen("/sys/fs/cgroup/cpu/cpu.cfs_quota_us", "r")) {
        long quota = -1, period = 0;
        if (fscanf(g, "%ld", &quota) != 1) quota = -1;
        fclose(g);
        if (FILE* h = fopen("/sys/fs/cgroup/cpu/cpu.cfs_period_us", "r")) { if (fscanf(h, "%ld", &period) != 1) period = 0; fclose(h); }
        if (quota > 0 && period > 0) { const int c = (int)(quota / period); if (c < n) n = c < 1 ? 1 : c; }
    }
    return n;
}
// How the groups of a slam2d_groups_* call are issued on this host (decided once).  One worker thread per group beyond the first
// halves the issue time of a scan -- when the threads have cores to run on: a worker polls for ~1-2 ms before it sleeps and the
// caller polls for its workers, i.e. TWO spinning threads per process, and a node runs one process per GPU.  With fewer than 3
// cores per local rank (8 ranks on a 16-core quota: the driver's box) the spinners would take the cores of Python, the HIP
// runtime's signal threads and RCCL's proxy threads: the groups are then issued from the calling thread.  In between (< 6) the
// threads stay but wait politely (short polls, sched_yield).
//   SLAM2D_GROUP_THREADS = 0 / 1 forces the choice; SLAM2D_LOCAL_RANKS (default: LOCAL_WORLD_SIZE, torchrun's, else 1) says how
//   many such processes share the host.
struct GroupPolicy { bool threads; bool polite; int cores, ranks; };
static const GroupPolicy& group_policy() {
    static const GroupPolicy pol = [] {
        GroupPolicy g;
        g.cores = effective_cores();
        const char* r = getenv("SLAM2D_LOCAL_RANKS");
        if (!r || atoi(r) < 1) r = getenv("LOCAL_WORLD_SIZE");
        g.ranks = r && atoi(r) >= 1 ? atoi(r) : 1;
        const int per = g.cores / g.ranks;
        g.threads = per >= 3;
        g.polite = per < 6;
        if (const char* e = getenv("SLAM2D_GROUP_THREADS")) g.threads = atoi(e) != 0;
        return g;
    }();
    return pol;
}

struct GroupWorker {
    std::atomic<int> state{0};           // 0 idle, 1 job posted, 2 done
    std::atomic<bool> sleeping{false};
    std::mutex m;
    std::condition_variable cv;
    int kind = 0, G = 0, i = 0, dev = 0, rc = 0;
    const Slam2dLidar* lidar = nullptr;
    const Slam2dGroup* groups = nullptr;
    const Slam2dScan* sc = nullptr;
    void loop() {
        int cur_dev = -1;
        const int poll = group_policy().polite ? 2000 : 200000;              // ~1-2 ms of polling (polite: ~15 us), then sleep
        for (;;) {
            int spins = 0;
            while (state.load(std::memory_order_acquire) != 1) {
                if (++spins < poll) {
                    // (a spinning thread that the scheduler has put on the caller's CPU must not hold it for a time slice: in the first
                    // bench process of two sessions the four-group closed loop ran 0.28 s per leg instead of 0.20, the one-group legs
                    // beside it did not.  sched_yield returns at once when nobody else wants the CPU)
                    if ((spins & 127) == 127) sched_yield(); else __builtin_ia32_pause();
                    continue;
                }
                std::unique_lock<std::mutex> lk(m);
                sleeping.store(true);
                cv.wait(lk, [&] { return state.load(std::memory_order_acquire) == 1; });
                sleeping.store(false);
            }
            if (dev != cur_dev) { (void)hipSetDevice(dev); cur_dev = dev; }
            rc = run_group_job(kind, lidar, groups, G, i, *sc);
            state.store(2, std::memory_order_release);
        }
    }
};
static GroupWorker* group_worker(int k) {
    static std::mutex mk;
    static GroupWorker* pool[64] = {};
    std::lock_guard<std::mutex> lk(mk);
    if (!pool[k]) {
        pool[k] = new GroupWorker;                       // (never freed: the thread sleeps until the process ends)
        std::thread(&GroupWorker::loop, pool[k]).detach();
    }
    return pool[k];
}
// One call at a time: the workers are a process-wide pool indexed by group number (ctypes releases the GIL, so two Python threads
// could otherwise post into the same worker).  A call may be left RUNNING (slam2d_groups_match_begin: the caller goes on while the
// workers issue the launches -- every group on a worker then, the descriptors copied so that the caller may rewrite its own); the
// next slam2d_groups_* call, or slam2d_groups_join, waits for it first and returns its error.
static std::mutex g_one_call;
static struct { int G = 0; int rc = 0; Slam2dScan scan; Slam2dGroup groups[64]; } g_begun;
static int join_locked() {
    const GroupPolicy& pol = group_policy();
    int rc = g_begun.rc;
    for (int i = 0; i < g_begun.G; ++i) {
        GroupWorker* w = group_worker(i);
        int spins = 0;
        while (w->state.load(std::memory_order_acquire) != 2) {
            if ((++spins & 127) == 127 || (pol.polite && spins > 256)) sched_yield(); else __builtin_ia32_pause();
        }
        if (!rc) rc = w->rc;
        w->state.store(0, std::memory_order_release);
    }
    g_begun.G = 0; g_begun.rc = 0;
    return rc;
}
static void post(GroupWorker* g, int kind, const Slam2dLidar* lidar, const Slam2dGroup* groups, int G, int i, const Slam2dScan* scan, int dev) {
    g->kind = kind; g->lidar = lidar; g->groups = groups; g->G = G; g->i = i; g->sc = scan; g->dev = dev;
    g->state.store(1, std::memory_order_seq_cst);
    if (g->sleeping.load()) { { std::lock_guard<std::mutex> lk(g->m); } g->cv.notify_one(); }
}
static int run_groups(int kind, const Slam2dLidar* lidar, const Slam2dGroup* groups, int32_t G, const Slam2dScan* scan, const bool leave_running = false) {
    std::lock_guard<std::mutex> serial(g_one_call);
    int rc = join_locked();
    if (rc) return rc;
    const GroupPolicy& pol = group_policy();
    if (!pol.threads || (G < 2 && !leave_running)) {
        for (int i = 0; i < G && !rc; ++i) rc = run_group_job(kind, lidar, groups, G, i, *scan);
        return rc;
    }
    int dev = 0;
    (void)hipGetDevice(&dev);
    if (leave_running) {
        g_begun.scan = *scan;
        for (int i = 0; i < G; ++i) g_begun.groups[i] = groups[i];
        for (int i = 0; i < G; ++i) post(group_worker(i), kind, lidar, g_begun.groups, G, i, &g_begun.scan, dev);
        g_begun.G = G;
        return 0;
    }
    for (int i = 1; i < G; ++i) post(group_worker(i), kind, lidar, groups, G, i, scan, dev);
    rc = run_group_job(kind, lidar, groups, G, 0, *scan);
    for (int i = 1; i < G; ++i) {
        GroupWorker* w = group_worker(i);
        int spins = 0;
        while (w->state.load(std::memory_order_acquire) != 2) {
            if ((++spins & 127) == 127 || (pol.polite && spins > 256)) sched_yield(); else __builtin_ia32_pause();
        }
        if (!rc) rc = w->rc;
        w->state.store(0, std::memory_order_release);
    }
    return rc;
}

int slam2d_groups_match_begin(const Slam2dLidar* lidar, const Slam2dGroup* groups, int32_t G, const Slam2dScan* scan) {
    const int rc = groups_check(lidar, groups, G, scan, false);
    return rc ? rc : run_groups(JOB_MATCH, lidar, groups, G, scan, true);
}

int slam2d_groups_join(void) {
    std::lock_guard<std::mutex> serial(g_one_call);
    return join_locked();
}

int slam2d_host_wait_seq(const uint32_t* h_seq, uint32_t want, double timeout_s) {
    if (!h_seq) return SLAM2D_E_BADARG;
    const auto t0 = std::chrono::steady_clock::now();
    const GroupPolicy& pol = group_policy();
    const bool polite = pol.polite || !pol.threads;        // (few cores per rank: the runtime's and RCCL's threads need them too)
    for (unsigned spins = 0;; ++spins) {
        if ((int32_t)(__atomic_load_n(h_seq, __ATOMIC_ACQUIRE) - want) >= 0) return 0;
        if ((spins & (polite ? 63u : 255u)) == (polite ? 63u : 255u)) sched_yield(); else __builtin_ia32_pause();
        if ((spins & 1023u) == 1023u && std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count() > timeout_s) return SLAM2D_E_TIMEOUT;
    }
}

/* how slam2d_groups_* issue their groups on this host: out[0] = effective cores, out[1] = local ranks assumed, out[2] = 1 if a
 * worker thread per group is used, out[3] = 1 if the threads wait politely */
int slam2d_group_policy(int32_t* out4) {
    if (!out4) return SLAM2D_E_BADARG;
    const GroupPolicy& g = group_policy();
    out4[0] = g.cores; out4[1] = g.ranks; out4[2] = g.threads ? 1 : 0; out4[3] = g.polite ? 1 : 0;
    return 0;
}

int slam2d_groups_match(const Slam2dLidar* lidar, const Slam2dGroup* groups, int32_t G, const Slam2dScan* scan) {
    const int rc = groups_check(lidar, groups, G, scan, false);
    return rc ? rc : run_groups(JOB_MATCH, lidar, groups, G, scan);
}

int slam2d_groups_commit(const Slam2dLidar* lidar, const Slam2dGroup* groups, int32_t G, const Slam2dScan* scan) {
    int rc = groups_check(lidar, groups, G, scan, true);
    if (!rc) rc = run_groups(JOB_COMMIT, lidar, groups, G, scan);     // (every ev_matched was recorded by the match call before this one)
    return rc ? rc : groups_merge(groups, G, *scan);
}

int slam2d_groups_step(const Slam2dLidar* lidar, const Slam2dGroup* groups, int32_t G, const Slam2dScan* scan) {
    int rc = groups_check(lidar, groups, G, scan, true);
    if (!rc && scan->abort_mask) return SLAM2D_E_BADARG;      // (an abort needs every match before any commit: use the two calls)
    if (!rc) rc = run_groups(JOB_STEP, lidar, groups, G, scan);
    return rc ? rc : groups_merge(groups, G, *scan);
}

int slam2d_weights_local(double* d_logw, const double* d_logconf, int32_t logconf_stride, int32_t N, double* d_part,
                         void* stream) {
    if (!d_logw || !d_part || N <= 0 || (d_logconf && logconf_stride < 1)) return SLAM2D_E_BADARG;
    k_weights_local<<<1, 256, 0, (hipStream_t)stream>>>(d_logw, d_logconf, logconf_stride, N, d_part);
    return launch_status();
}

int slam2d_weights_merge(double* d_logw, int32_t N, const double* d_parts, int32_t world, int64_t total_particles,
                         double* d_w, double* d_stats, void* stream) {
    if (!d_logw || !d_parts || !d_w || !d_stats || N <= 0 || world <= 0 || total_particles < N) return SLAM2D_E_BADARG;
    k_weights_merge<<<1, 256, 0, (hipStream_t)stream>>>(d_logw, N, d_parts, world, (double)total_particles, d_w, d_stats, nullptr, 0, 0u);
    return launch_status();
}

int slam2d_norm_gate(uint32_t* d_norm_sync, int32_t G, void* stream) {
    if (!d_norm_sync || G <= 0 || G > SLAM2D_SYNC_MAX_GROUPS) return SLAM2D_E_BADARG;
    k_norm_gate<<<1, 64, 0, (hipStream_t)stream>>>(d_norm_sync, G);
    return launch_status();
}

int slam2d_weights_merge_publish(double* d_logw, int32_t N, const double* d_parts, int32_t world, int64_t total_particles,
                                 double* d_w, double* d_stats, uint32_t* d_norm_sync, void* stream) {
    if (!d_logw || !d_parts || !d_w || !d_stats || !d_norm_sync || N <= 0 || world <= 0 || total_particles < N) return SLAM2D_E_BADARG;
    k_weights_merge<<<1, 256, 0, (hipStream_t)stream>>>(d_logw, N, d_parts, world, (double)total_particles, d_w, d_stats, nullptr, 0, 0u, d_norm_sync);
    return launch_status();
}

int slam2d_weights_merge_publish_report(double* d_logw, int32_t N, const double* d_parts, int32_t world, int64_t total_particles,
                                        double* d_w, double* d_stats, uint32_t* d_norm_sync, const double* d_pack, double* h_pack,
                                        int32_t pack_doubles, uint32_t* h_seq, uint32_t report_seq, void* stream) {
    if (!d_logw || !d_parts || !d_w || !d_stats || !d_norm_sync || N <= 0 || world <= 0 || total_particles < N) return SLAM2D_E_BADARG;
    if (!d_pack || !h_pack || !h_seq || pack_doubles <= 0) return SLAM2D_E_BADARG;
    k_weights_merge<<<1, 256, 0, (hipStream_t)stream>>>(d_logw, N, d_parts, world, (double)total_particles, d_w, d_stats, nullptr, 0, 0u, d_norm_sync,
                                                        d_pack, h_pack, pack_doubles, h_seq, report_seq);
    return launch_status();
}

int slam2d_gather_maps(const Slam2dMap* d_src, const Slam2dMap* d_dst, const int32_t* d_index, int32_t P,
                       int64_t cells_per_map, void* stream) {
    if (!d_src || !d_dst || !d_index || P <= 0 || cells_per_map <= 0) return SLAM2D_E_BADARG;
    const int gx = (int)((cells_per_map + 256 * 8 - 1) / (256 * 8));
    k_gather_maps<<<dim3(gx < 1 ? 1 : gx, P), 256, 0, (hipStream_t)stream>>>(d_src, d_dst, d_index);
    return launch_status();
}

int slam2d_map_refresh_bits(const Slam2dMap* d_maps, const int32_t* d_index, int32_t n, void* stream) {
    if (!d_maps || n <= 0) return SLAM2D_E_BADARG;
    k_refresh_bits<<<dim3(1024, n), 256, 0, (hipStream_t)stream>>>(d_maps, d_index);
    return launch_status();
}

int slam2d_map_image(const Slam2dMap* d_maps, int32_t p, int32_t x0, int32_t x1, int32_t y0, int32_t y1, int32_t flipud,
                     double* d_out, uint8_t* d_out_u8, void* stream) {
    if (!d_maps || p < 0 || x0 < 0 || y0 < 0 || x1 <= x0 || y1 <= y0 || (!d_out && !d_out_u8)) return SLAM2D_E_BADARG;
    const long long n = (long long)(x1 - x0) * (y1 - y0);
    long long blocks = (n + 256 * 4 - 1) / (256 * 4);
    if (blocks > 65535) blocks = 65535;
    k_map_image<<<(unsigned)blocks, 256, 0, (hipStream_t)stream>>>(d_maps, p, x0, y0, x1 - x0, y1 - y0, flipud, d_out, d_out_u8);
    return launch_status();
}

int slam2d_map_fill(uint32_t* d_cells, int64_t n, uint32_t value, void* stream) {
    if (!d_cells || n <= 0) return SLAM2D_E_BADARG;
    long long blocks = (n + 256 * 8 - 1) / (256 * 8);
    if (blocks > 65535) blocks = 65535;
    k_fill<<<(unsigned)blocks, 256, 0, (hipStream_t)stream>>>(d_cells, (long long)n, value);
    return launch_status();
}

// expandOccupancyGrid (Utils/OccupancyGrid.py:59-100) on the device, once per growth SEQUENCE: the new count array in one pass --
// old content at its shifted place (np.insert / np.append of fresh columns / rows: :70-71, :81-82), SLAM2D_INIT_CELL everywhere
// else, the pitch padding included -- and the new occupancy bits from the cells as they are written (k_refresh_bits' test).
// One wave = 64 consecutive cells of a row: a 256-byte read where the old map covers them, a 256-byte write, one ballot.
__global__ __launch_bounds__(256) void k_map_grow(const Slam2dMap o, const Slam2dMap n, const int d_row, const int d_col) {
    const int lane = threadIdx.x & 63;
    const int groups_per_row = (n.pitch + 63) >> 6;
    const long long ngroups = (long long)n.rows * groups_per_row;
    for (long long g = (long long)blockIdx.x * 4 + (threadIdx.x >> 6); g < ngroups; g += (long long)gridDim.x * 4) {
        const int row = (int)(g / groups_per_row), c0 = (int)(g - (long long)row * groups_per_row) << 6;
        const int col = c0 + lane;
        const int orow = row - d_row, ocol = col - d_col;
        const bool inside = orow >= 0 && orow < o.rows && ocol >= 0 && ocol < o.cols && col < n.cols;
        bool occ = false;
        if (n.wide) {
            unsigned long long v = ((unsigned long long)(SLAM2D_INIT_CELL >> 16) << 32) | (SLAM2D_INIT_CELL & 0xffffu);
            if (inside) v = reinterpret_cast<const unsigned long long*>(o.cells)[(size_t)orow * o.pitch + ocol];
            if (col < n.pitch) reinterpret_cast<unsigned long long*>(n.cells)[(size_t)row * n.pitch + col] = v;
            occ = col < n.cols && 2ull * (v >> 32) > (v & 0xffffffffull);
        } else {
            uint32_t v = SLAM2D_INIT_CELL;
            if (inside) v = o.cells[(size_t)orow * o.pitch + ocol];
            if (col < n.pitch) n.cells[(size_t)row * n.pitch + col] = v;
            occ = col < n.cols && 2u * (v >> 16) > (v & 0xffffu);                   // :29-31
        }
        const unsigned long long mask = __ballot(occ);
        if (lane < 2 && (c0 >> 5) + lane < n.bits_pitch)
            n.occ_bits[(size_t)row * n.bits_pitch + (c0 >> 5) + lane] = (uint32_t)(mask >> (32 * lane));
    }
}

int slam2d_map_grow(const Slam2dMap* old_map, const Slam2dMap* new_map, int32_t d_row, int32_t d_col, void* stream) {
    if (!old_map || !new_map || !old_map->cells || !new_map->cells || !new_map->occ_bits || d_row < 0 || d_col < 0) return SLAM2D_E_BADARG;
    if (old_map->wide != new_map->wide || new_map->rows < old_map->rows + d_row || new_map->cols < old_map->cols + d_col ||
        new_map->pitch < new_map->cols || new_map->bits_pitch * 32 < new_map->cols) return SLAM2D_E_BADARG;
    const long long ngroups = (long long)new_map->rows * ((new_map->pitch + 63) >> 6);
    long long blocks = (ngroups + 3) / 4;
    if (blocks > 8192) blocks = 8192;
    k_map_grow<<<(unsigned)blocks, 256, 0, (hipStream_t)stream>>>(*old_map, *new_map, d_row, d_col);
    return launch_status();
}

// ---- stage profiling ----
int slam2d_prof_enable(uint32_t stage_mask, int32_t capacity) {
    if (capacity <= 0) return SLAM2D_E_BADARG;
    for (int st = 0; st < SLAM2D_STAGE_COUNT; ++st) {
        StageProf& p = g_prof[st];
        if (!((stage_mask >> st) & 1u)) continue;
        if (p.capacity < capacity) {
            for (int i = 0; i < p.capacity; ++i) { (void)hipEventDestroy(p.start[i]); (void)hipEventDestroy(p.stop[i]); }
            delete[] p.start; delete[] p.stop;
            p.start = new hipEvent_t[capacity]; p.stop = new hipEvent_t[capacity];
            for (int i = 0; i < capacity; ++i) {
                hipError_t e = hipEventCreate(&p.start[i]);
                if (e == hipSuccess) e = hipEventCreate(&p.stop[i]);
                if (e != hipSuccess) { p.capacity = 0; return (int)e; }
            }
            p.capacity = capacity;
        }
        p.used = 0;
        p.seen = 0;
    }
    g_prof_mask = stage_mask;
    return 0;
}

int slam2d_prof_every(int32_t every) {
    if (every < 1) return SLAM2D_E_BADARG;
    g_prof_every = every;
    return 0;
}

int slam2d_prof_collect(int32_t stage, double* total_ms, int32_t* launches) {
    if (stage < 0 || stage >= SLAM2D_STAGE_COUNT || !total_ms || !launches) return SLAM2D_E_BADARG;
    StageProf& p = g_prof[stage];
    double tot = 0.0;
    for (int i = 0; i < p.used; ++i) {
        hipError_t e = hipEventSynchronize(p.stop[i]);
        if (e != hipSuccess) return (int)e;
        float ms = 0.f;
        e = hipEventElapsedTime(&ms, p.start[i], p.stop[i]);
        if (e != hipSuccess) return (int)e;
        tot += ms;
    }
    *total_ms = tot;
    *launches = p.used;
    p.used = 0;
    return 0;
}

void slam2d_prof_disable(void) { g_prof_mask = 0; }

// cos / sin exactly as k_endpoints evaluates them for the beam angles (ocml fp64): lets the tests measure the
// distance to NumPy's libm on the same angles (deviation (i))
__global__ void k_sincos(const double* __restrict__ a, int n, double* c, double* s) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) { c[i] = cos(a[i]); s[i] = sin(a[i]); }
}
int slam2d_device_sincos(const double* d_angles, int32_t n, double* d_cos, double* d_sin, void* stream) {
    if (!d_angles || !d_cos || !d_sin || n <= 0) return SLAM2D_E_BADARG;
    k_sincos<<<cdiv(n, 256), 256, 0, (hipStream_t)stream>>>(d_angles, n, d_cos, d_sin);
    return launch_status();
}

#ifdef SLAM2D_DEBUG_CLOCK
int slam2d_debug_clock(long long* out64) {
    return (int)hipMemcpyFromSymbol(out64, HIP_SYMBOL(g_dbg_clock), sizeof(long long) * 64);
}
#endif

// ---- ordering between streams (no timing): events a host driver uses to chain particle groups on several streams ----
void* slam2d_event_create(void) {
    hipEvent_t e;
    if (hipEventCreateWithFlags(&e, hipEventDisableTiming) != hipSuccess) return nullptr;
    return (void*)e;
}
void slam2d_event_destroy(void* event) { if (event) (void)hipEventDestroy((hipEvent_t)event); }
int slam2d_event_record(void* event, void* stream) { return event ? (int)hipEventRecord((hipEvent_t)event, (hipStream_t)stream) : SLAM2D_E_BADARG; }
int slam2d_stream_wait_event(void* stream, void* event) { return event ? (int)hipStreamWaitEvent((hipStream_t)stream, (hipEvent_t)event, 0) : SLAM2D_E_BADARG; }

// ---- a batch of streams for particle groups ----
// Which HARDWARE queue a HIP stream sits on decides whether two groups overlap or take turns: the runtime keeps at most
// GPU_MAX_HW_QUEUES of them (4 unless the application sets more before its first HIP call) and decides itself which one a new stream
// gets.  Creating the streams in one batch and using each once at once is not enough: at four queues the nine streams of a batch
// came out with the four group streams on TWO queues, two groups alternating on each (round 8: config 2 in four groups 0.185 ms per
// step against 0.11 on a queue each; round 5 had seen the same with pooled streams: 0.42-0.50 s against 0.21 s in the closed loop).
// So the batch is PLACED BY MEASUREMENT.  The probe: k_spin (one wave, busy for PROBE_SPAN_TICKS of the 100 MHz wall clock, or
// PROBE_SPIN_CAP iterations whatever the clock does) on stream a, then k_stamp on stream b, both synchronised, ticks read from a
// pinned buffer.  The stamp precedes the spin's end only if b's queue is not a's -- one in-order queue starts nothing of b before a's
// kernel ends, so "distinct" is never wrong; "same" can be an unlucky moment (the host descheduled between the two launches, a busy
// device) and is believed only after PROBE_TRIES times.  No kernel waits for another; each ends by itself.
// Candidates are sorted into queue classes against one representative per class (candidates x classes probes, not all pairs), in
// three tiers: (0) the n streams created as before; (1) up to n further non-blocking streams, one at a time, while fewer than four
// classes are known; (2) up to n streams at the device's greatest stream priority -- the runtime keeps a queue pool per priority (round 8:
// measured so at one to three queues); the probe decides whether that holds.  Placement: out[1..4] (the group streams of a four- and of a two-group run) on pairwise distinct
// queues; then out[0] (the normaliser's, busy beside two groups on a sharded rank) not on the queue of out[1] or out[2]; the rest in
// creation order.  Tier-0 streams are preferred in creation order, so a batch whose streams already sit on distinct queues (eight
// queues) comes out exactly as created.  Fewer than four classes after all tiers: the best placement found, not an error.
// Bound: at most 3n candidates, each probed against at most PROBE_MAX_CLASSES representatives, a "same" up to PROBE_TRIES times:
// 3n x 8 x 3 probes of ~0.2 ms (n = 9: 648 probes, 0.13 s; measured: profiles/r08_group_queues.md) -- once per process and device.
constexpr long long PROBE_SPAN_TICKS = 15000;        // 150 us of the 100 MHz constant clock
constexpr int PROBE_SPIN_CAP = 200000;               // clock reads: the span needs a few thousand; a stuck clock ends after a few ms
constexpr int PROBE_TRIES = 3, PROBE_MAX_CLASSES = 8;
__global__ void k_touch() {}
__global__ void k_spin(long long* ticks) {
    if (threadIdx.x != 0) return;
    const long long t0 = (long long)wall_clock64();
    long long t = t0;
    for (int i = 0; i < PROBE_SPIN_CAP && t - t0 < PROBE_SPAN_TICKS; ++i) t = (long long)wall_clock64();
    ticks[0] = t;
}
__global__ void k_stamp(long long* ticks) { if (threadIdx.x == 0) ticks[1] = (long long)wall_clock64(); }

namespace {
struct StreamBatch {                                 // the last batch of slam2d_streams_create, for slam2d_streams_queue_classes
    std::mutex m;
    void* stream[64];
    int32_t cls[64];
    int32_t n = 0, n_classes = 0;
    int32_t stats[6] = {0, 0, 0, 0, 0, 0};           // tier, probes, created, destroyed, microseconds, streams placed on a shared queue among out[1..4]
} g_batch;

// 1: b's queue is not a's; 0: no overlap seen in PROBE_TRIES probes; < 0: -hipError_t
int probe_distinct(hipStream_t a, hipStream_t b, long long* ticks, int32_t* probes) {
    for (int t = 0; t < PROBE_TRIES; ++t) {
        ticks[0] = 0; ticks[1] = 0;
        k_spin<<<1, 64, 0, a>>>(ticks);
        k_stamp<<<1, 64, 0, b>>>(ticks);
        hipError_t e = hipGetLastError();
        const hipError_t ea = hipStreamSynchronize(a), eb = hipStreamSynchronize(b);
        if (e == hipSuccess) e = ea != hipSuccess ? ea : eb;
        if (e != hipSuccess) return -(int)e;
        ++*probes;
        const volatile long long* v = ticks;
        if (v[1] < v[0]) return 1;
    }
    return 0;
}
}  // namespace

int slam2d_streams_create(void** out, int32_t n) {
    if (!out || n <= 0 || n > 64) return SLAM2D_E_BADARG;
    constexpr int MAXC = 3 * 64;
    hipStream_t cand[MAXC];
    int cls[MAXC], nc = 0, ncls = 0, tier = 0;
    hipStream_t rep[PROBE_MAX_CLASSES];
    int32_t probes = 0, created = 0, destroyed = 0;
    long long* ticks = nullptr;
    const auto t_begin = std::chrono::steady_clock::now();
    hipError_t err = hipSuccess;
    auto fail = [&](hipError_t e) {
        for (int j = 0; j < nc; ++j) (void)hipStreamDestroy(cand[j]);
        if (ticks) (void)hipHostFree(ticks);
        return (int)e;
    };
    // classify cand[i]: the class of the first representative it does not overlap with, or a new class (beyond PROBE_MAX_CLASSES: the last)
    auto classify = [&](int i) -> hipError_t {
        for (int k = 0; k < ncls; ++k) {
            const int d = probe_distinct(rep[k], cand[i], ticks, &probes);
            if (d < 0) return (hipError_t)(-d);
            if (d == 0) { cls[i] = k; return hipSuccess; }
        }
        if (ncls < PROBE_MAX_CLASSES) { rep[ncls] = cand[i]; cls[i] = ncls++; }
        else cls[i] = PROBE_MAX_CLASSES - 1;
        return hipSuccess;
    };
    // tier 0: the batch as it has always been made
    for (int i = 0; i < n; ++i) {
        hipStream_t st;
        const hipError_t e = hipStreamCreateWithFlags(&st, hipStreamNonBlocking);
        if (e != hipSuccess) return fail(e);
        cand[nc++] = st; ++created;
        k_touch<<<1, 64, 0, st>>>();                   // (first use = queue assignment, in creation order)
    }
    for (int i = 0; i < n; ++i) (void)hipStreamSynchronize(cand[i]);
    if ((err = hipGetLastError()) != hipSuccess) return fail(err);
    if ((err = hipHostMalloc((void**)&ticks, 2 * sizeof(long long), hipHostMallocPortable)) != hipSuccess) { ticks = nullptr; return fail(err); }
    // the group streams are looked for from element 1 on, so classify in that order: 1 .. n-1, then 0
    for (int j = 0; j < n; ++j) if ((err = classify((j + 1) % n)) != hipSuccess) return fail(err);
    const int want = n - 1 < 4 ? n - 1 : 4;            // distinct queues asked for
    // tier 1: further plain streams; tier 2: streams at the greatest priority
    int lo = 0, hi = 0;
    (void)hipDeviceGetStreamPriorityRange(&lo, &hi);
    for (int t = 1; t <= 2 && ncls < want; ++t) {
        if (t == 2 && hi == 0) break;                  // (no second priority level on this device)
        for (int j = 0; j < n && ncls < want; ++j) {
            hipStream_t st;
            const hipError_t e = t == 1 ? hipStreamCreateWithFlags(&st, hipStreamNonBlocking) : hipStreamCreateWithPriority(&st, hipStreamNonBlocking, hi);
            if (e != hipSuccess) return fail(e);
            cand[nc++] = st; ++created;
            k_touch<<<1, 64, 0, st>>>();
            (void)hipStreamSynchronize(st);
            const int before = ncls;
            if ((err = classify(nc - 1)) != hipSuccess) return fail(err);
            if (ncls > before) tier = t;
        }
    }
    (void)hipHostFree(ticks); ticks = nullptr;
    // placement
    int pick[64], used[MAXC] = {0};
    for (int i = 0; i < n; ++i) pick[i] = -1;
    bool cls_used[PROBE_MAX_CLASSES] = {false};
    int order[MAXC];                                   // candidates in the order of preference: 1 .. n-1, 0, then the later tiers
    for (int j = 0; j < n; ++j) order[j] = (j + 1) % n;
    for (int j = n; j < nc; ++j) order[j] = j;
    for (int s = 1; s <= want; ++s)                    // out[1..4]: one stream of each class, while classes last
        for (int j = 0; j < nc; ++j) {
            const int c = order[j];
            if (!used[c] && !cls_used[cls[c]]) { pick[s] = c; used[c] = 1; cls_used[cls[c]] = true; break; }
        }
    // out[0]: a free stream of a class no group stream has; else of a class other than out[1]'s and out[2]'s (moving that class's group
    // stream to out[3] / out[4] where it sits at out[1] / out[2]); candidate 0 first
    {
        int best = -1, best_rank = 3;
        for (int j = -1; j < nc; ++j) {
            const int c = j < 0 ? 0 : order[j];
            if (used[c]) continue;
            int rank = cls_used[cls[c]] ? 1 : 0;
            if (rank == 1) {                           // its class holds a group stream: usable if that stream can sit at out[3] or out[4]
                int at = 0, groups = 0;
                for (int s = 1; s <= want; ++s) if (pick[s] >= 0) { ++groups; if (cls[pick[s]] == cls[c]) at = s; }
                if (at <= 2 && groups < 3) rank = 2;
            }
            if (rank < best_rank) { best = c; best_rank = rank; }
        }
        if (best >= 0) {
            pick[0] = best; used[best] = 1;
            for (int s = 1; s <= 2 && s <= want; ++s)
                if (pick[s] >= 0 && cls[pick[s]] == cls[best])
                    for (int u = want; u >= 3; --u)
                        if (pick[u] >= 0 && cls[pick[u]] != cls[best]) { const int tmp = pick[s]; pick[s] = pick[u]; pick[u] = tmp; break; }
        }
    }
    int shared = 0, groups_on[PROBE_MAX_CLASSES] = {0};
    for (int s = 1; s <= want; ++s) if (pick[s] >= 0) ++groups_on[cls[pick[s]]];
    for (int s = 0; s < n; ++s) {                      // whatever is still open: the free stream on the queue with the fewest group streams
        if (pick[s] >= 0) continue;
        int best = -1;
        for (int j = 0; j < nc; ++j) {
            const int c = order[j];
            if (!used[c] && (best < 0 || (s >= 1 && s <= 4 && groups_on[cls[c]] < groups_on[cls[best]]))) best = c;
        }
        pick[s] = best; used[best] = 1;
        if (s >= 1 && s <= 4 && groups_on[cls[best]]++ > 0) ++shared;
    }
    for (int j = 0; j < nc; ++j) if (!used[j]) { (void)hipStreamDestroy(cand[j]); ++destroyed; }
    {
        std::lock_guard<std::mutex> lk(g_batch.m);
        g_batch.n = n; g_batch.n_classes = ncls;
        for (int i = 0; i < n; ++i) { out[i] = (void*)cand[pick[i]]; g_batch.stream[i] = out[i]; g_batch.cls[i] = cls[pick[i]]; }
        g_batch.stats[0] = tier; g_batch.stats[1] = probes; g_batch.stats[2] = created; g_batch.stats[3] = destroyed;
        g_batch.stats[4] = (int32_t)std::chrono::duration_cast<std::chrono::microseconds>(std::chrono::steady_clock::now() - t_begin).count();
        g_batch.stats[5] = shared;
    }
    return launch_status();
}
// The queue class of each of `streams` in the last batch of slam2d_streams_create (-1: not of that batch) and the number of classes
// that batch found.  stats (NULL, or 6 words): the tier that supplied the last class (0 the plain batch, 1 further streams, 2 priority
// streams), probes run, candidate streams created, candidates destroyed again, microseconds the batch took, group streams (elements
// 1..4) that had to share a queue.  No HIP call: works without a device.
int slam2d_streams_queue_classes(void* const* streams, int32_t n, int32_t* out_class, int32_t* n_classes, int32_t* stats) {
    if (!streams || !out_class || !n_classes || n <= 0 || n > 64) return SLAM2D_E_BADARG;
    std::lock_guard<std::mutex> lk(g_batch.m);
    for (int i = 0; i < n; ++i) {
        out_class[i] = -1;
        for (int j = 0; j < g_batch.n; ++j) if (streams[i] && g_batch.stream[j] == streams[i]) { out_class[i] = g_batch.cls[j]; break; }
    }
    *n_classes = g_batch.n_classes;
    if (stats) for (int i = 0; i < 6; ++i) stats[i] = g_batch.stats[i];
    return 0;
}
void slam2d_stream_destroy(void* stream) { if (stream) (void)hipStreamDestroy((hipStream_t)stream); }

// ---- plain event timer ----
struct Timer { hipEvent_t a, b; };
void* slam2d_timer_create(void) {
    Timer* t = new Timer;
    if (hipEventCreate(&t->a) != hipSuccess || hipEventCreate(&t->b) != hipSuccess) { delete t; return nullptr; }
    return t;
}
void slam2d_timer_destroy(void* timer) {
    if (!timer) return;
    Timer* t = (Timer*)timer;
    (void)hipEventDestroy(t->a); (void)hipEventDestroy(t->b);
    delete t;
}
int slam2d_timer_start(void* timer, void* stream) { return timer ? (int)hipEventRecord(((Timer*)timer)->a, (hipStream_t)stream) : SLAM2D_E_BADARG; }
int slam2d_timer_stop(void* timer, void* stream) { return timer ? (int)hipEventRecord(((Timer*)timer)->b, (hipStream_t)stream) : SLAM2D_E_BADARG; }
int slam2d_timer_elapsed_ms(void* timer, float* ms) {
    if (!timer || !ms) return SLAM2D_E_BADARG;
    Timer* t = (Timer*)timer;
    hipError_t e = hipEventSynchronize(t->b);
    if (e != hipSuccess) return (int)e;
    return (int)hipEventElapsedTime(ms, t->a, t->b);
}

}  // extern "C"
