/*
 * slam2d.h -- C ABI of libslam2d_hip.so: MI355X (gfx950) kernels for the 2-D lidar
 * FastSLAM hot path of xiaofeng419/SLAM-2D-LIDAR-SCAN.
 *
 * The reference is pure Python and has no FFI layer; its boundary for this path is
 * the class surface of Utils/OccupancyGrid.py:OccupancyGrid and
 * Utils/ScanMatcher_OGBased.py:ScanMatcher as driven by Algorithm/FastSlam.py
 * (SURVEY.md section 8b).  Each entry point below replaces the body of one of
 * those methods for a batch of P particles; the Python classes in
 * slam-2d-lidar-scan_amd/ keep the reference's constructor/method/attribute
 * surface and call these through ctypes (INTEGRATION.md shows the binding).
 *
 * Conventions
 *   - plain C: PODs, raw pointers, sizes; no C++ or torch types.
 *   - every pointer named d_* (and every pointer inside the structs) is DEVICE memory
 *     owned by the caller (the Python side allocates it as torch tensors);
 *     the library allocates no device memory and keeps no state between calls -- except the sleeping host threads of
 *     slam2d_groups_* (one per particle group beyond the first, created on first use; SLAM2D_GROUP_THREADS=0: none),
 *     the event pairs of slam2d_prof_* and the queue classes of the last slam2d_streams_create batch (which also owns, for
 *     its duration, two pinned words for its probe).  The slam2d_groups_* calls are not re-entrant (one caller at a time).
 *   - every call enqueues work on `stream` (a hipStream_t passed as void*) and returns
 *     without synchronising; results are ordered after the call on that stream.
 *   - return value: 0 on success, otherwise a hipError_t code (> 0) or a
 *     SLAM2D_E_* code (< 0).  No exceptions cross the boundary.
 *   - data-dependent faults (window outside the map, count overflow, cell list
 *     overflow) are reported by OR-ing SLAM2D_F_* bits into d_flags[p]; the offending
 *     access is skipped, never performed out of bounds.
 *   - row-major everywhere; images are [rows = y][cols = x].
 *
 * Search field format (Slam2dLevel.field, one uint32 per field cell): the reference's
 *   probSP (Utils/ScanMatcher_OGBased.py:41-45) holds values in [probMin, 0]; the field
 *   stores the non-negative fixed-point COST  c = rint(-probSP * cost_scale),
 *   cost_scale = 2^k chosen per level so that -probMin * 2^k < 2^32 (k = 31 for the
 *   reference's parameters: resolution 4.7e-10, ~30x finer than float32 at the same
 *   4 bytes).  Pose scores are then exact integer sums (uint64), so they do not depend
 *   on summation order and exact ties of the reference stay exact ties.
 *
 * Cell format of a particle's map (one uint32 per cell):
 *     bits 31..16 = occupancyGridVisited count, bits 15..0 = occupancyGridTotal count
 *   (reference: two float64 arrays initialised to 1 and 2, Utils/OccupancyGrid.py:13-14;
 *    hit: visited += 2, total += 2; miss: total += 1, :148-152).  A cell is occupied
 *   iff 2*visited > total (== visited/total > 0.5, Utils/ScanMatcher_OGBased.py:29-31).
 *   That format holds 32766 observations of one cell; a map that may exceed it is kept in 64-bit cells
 *   (Slam2dMap.wide) -- the Python side promotes a map before that can happen; on a narrow map the update
 *   kernel raises SLAM2D_F_COUNT_OVERFLOW instead of wrapping.
 */
#ifndef SLAM2D_H
#define SLAM2D_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SLAM2D_ABI_VERSION 18
#define SLAM2D_SPOKE_BAND 16         /* radial band width of the beam-major spoke table, in cells */

/* library error codes (negative; positive values are hipError_t) */
#define SLAM2D_E_BADARG   (-1)
#define SLAM2D_E_TOOLARGE (-2)   /* a size exceeds a compiled-in limit */
#define SLAM2D_E_TIMEOUT  (-3)   /* slam2d_host_wait_seq: the device did not publish the awaited scan in time */

/* per-particle fault bits OR-ed into d_flags[p] */
#define SLAM2D_F_WINDOW_OUTSIDE_MAP 0x01u  /* search window not inside the map: grow first (checkAndExapndOG) */
#define SLAM2D_F_FIELD_INDEX        0x02u  /* an occupied cell mapped outside the field (reference: IndexError) */
#define SLAM2D_F_ENDPOINT_OUTSIDE   0x04u  /* a beam endpoint +/- search radius left the field */
#define SLAM2D_F_UPDATE_OUTSIDE_MAP 0x08u  /* map update touched a cell outside the map */
#define SLAM2D_F_COUNT_OVERFLOW     0x10u  /* a 16-bit count would overflow */
#define SLAM2D_F_FLOOR_REDO         0x20u  /* informational: field minimum != analytic floor, clamp pass redone */
#define SLAM2D_F_SYNC_TIMEOUT       0x40u  /* a device-side wait of the groups' normaliser / gates (d_norm_sync) gave up after its bound */
#define SLAM2D_F_SCAN_VOIDED        0x80u  /* informational, in a voided scan's fault-bit SNAPSHOT only (never in d_flags): the commit did nothing
                                              on the device (abort_mask).  With SLAM2D_F_SYNC_TIMEOUT beside it the scan is intact and may be
                                              run again (the gate gave up BEFORE anything was written); without this bit a timeout is fatal */

#define SLAM2D_F_UPDATE_CELL_COLLISION 0x100u /* slam2d_grid_update*: two adjacent window columns (rows) of a particle round to ONE map
                                              index (a pose on a half cell: rint's ties-to-even) -- the reference adds once per
                                              statement there, a per-cell update cannot.  The particle's map is not touched by that
                                              launch.  slam2d_map_scans is exact at such poses */

#define SLAM2D_INIT_CELL 0x00010002u       /* visited = 1, total = 2 */
#define SLAM2D_MAX_BLUR_RADIUS 16
#define SLAM2D_MAX_BEAMS 2048
#define SLAM2D_SYNC_WORDS 4            /* arrival counters per particle in Slam2dLevel.sync */

/* One particle's map (device-resident).  X[cols] / Y[rows] are the stored cell-centre
 * coordinates (reference OccupancyGridX[0, :] / OccupancyGridY[:, 0]; rank-1 by
 * construction, growth included -- Utils/OccupancyGrid.py:12,83-85).  lim_* mirror
 * mapXLim / mapYLim (:19-20,86-89). */
typedef struct {
    uint32_t*     cells;     /* [rows][pitch] */
    const double* X;         /* [cols] */
    const double* Y;         /* [rows] */
    int32_t rows, cols, pitch, bits_pitch;
    double  lim_x0, lim_x1, lim_y0, lim_y1;
    uint32_t*     occ_bits;  /* [rows][bits_pitch] 1 bit per cell: occupied (2*visited > total).  Kept in
                                step by slam2d_grid_update; after any other write to `cells` call
                                slam2d_map_refresh_bits.  The field build reads only these bits. */
    int32_t wide;            /* 0: cells are uint32 (visited << 16 | total).  1: cells are uint64 [rows][pitch] (visited << 32 | total),
                                `cells` points at them: the format of a map whose counts no longer fit 16 bits (a cell observed
                                more than ~32 000 times; the reference's float64 counts never saturate).  The host promotes a map
                                BEFORE an update could overflow it (it knows an upper bound: every update adds at most 2) */
    int32_t _pad;
} Slam2dMap;

/* Lidar + polar spoke lookup table shared by all particles
 * (Utils/OccupancyGrid.py:22-57). */
typedef struct {
    double unit;             /* unitGridSize */
    double max_range;        /* lidarMaxRange */
    double fov;              /* lidarFOV */
    double wall_half;        /* wallThickness / 2 */
    int32_t beams;           /* numSamplesPerRev */
    int32_t num_spokes;      /* numSpokes */
    int32_t spoke_start;     /* spokesStartIdx */
    int32_t lut_w;           /* W = 2*int(max_range/unit)+1 */
    const double*   lut_xs;  /* [W]  linspace(-R, R, W) */
    /* radByX / radByY / radByR (:47-57): the window cells of every spoke.  The cells of a spoke are
     * ordered by radial band -- SLAM2D_SPOKE_BAND consecutive values of floor(r / unit) -- and row-major
     * inside a band; a beam touches the bands up to the one that holds range + wallThickness/2 */
    const int32_t*  spoke_band;  /* [num_spokes][num_bands + 1] index of each band's first cell (absolute) */
    const uint32_t* spoke_cells; /* [W*W] (window row << 16) | window column */
    const double*   spoke_r;     /* [W*W] radius of that cell */
    int32_t num_bands;           /* floor(max r / unit) / SLAM2D_SPOKE_BAND + 1 */
    int32_t _pad;
    double lut_xs_step;          /* 2*max_range/(W-1) when lut_xs[j] == j*lut_xs_step - max_range bit for bit
                                    (last element max_range), as numpy.linspace computes it; 0: use lut_xs */
} Slam2dLidar;

/* Geometry of one particle's search field at one level, written by
 * slam2d_field_build and read by slam2d_sweep. */
typedef struct {
    double xlo, ylo;         /* xRangeList[0], yRangeList[0] */
    double xhi, yhi;
    double cx, cy;           /* window centre (the pose estimate) */
    double field_min;        /* min of the blurred field (probMin) */
    int32_t fh, fw;          /* field rows / cols actually used (<= fmax) */
    int32_t mx0, mx1;        /* map column window [mx0, mx1) */
    int32_t my0, my1;        /* map row window    [my0, my1) */
    int32_t redo;            /* 1 = the clamp was redone with the measured minimum */
    int32_t min_known;       /* 1 = some tile of the frame is free, so field_min is the analytic floor */
    double field_max;        /* largest value of the (clamped) field over the tiles built at this call */
} Slam2dFrame;

/* Reduction of the 64*R consecutive cube entries one wave of the sweep scored. */
typedef struct {
    double  max;             /* largest score of the chunk (NaN if the chunk holds a NaN) */
    double  sumexp;          /* sum exp(score - max) over the chunk */
    int32_t argmax;          /* flat cube index of max (lowest on ties; first NaN if any) */
    int32_t has_nan;
} Slam2dPartial;

/* One search level (coarse or fine) for P particles: parameters + workspaces.
 * Reference: the two halves of ScanMatcher.matchScan,
 * Utils/ScanMatcher_OGBased.py:53-60 (coarse) and :65-73 (fine). */
typedef struct {
    /* ---- field build (frameSearchSpace + generateProbSearchSpace, :20-45) ---- */
    double step;             /* unitLength: coarseFactor*unit or unit */
    double reach;            /* 1.1*lidarMaxRange + searchRadius (ctor value, both levels) */
    double log_miss;         /* log(missMatchProb) of this level */
    double floor_value;      /* analytic field minimum: blur of an all-free neighbourhood */
    double cost_scale;       /* 2^k: field stores rint(-probSP * cost_scale) as uint32 */
    int32_t blur_radius;     /* int(4*sigma + 0.5) */
    int32_t fmax;            /* max field rows/cols over particles: int(2*reach/step) + 2 */
    int32_t fpitch;          /* row pitch (elements) of field / occ images, >= fmax */
    int32_t wmax;            /* max map-window edge: int(2*reach/unit) + 3 */
    const double* blur_w;    /* [2*blur_radius+1] normalised Gaussian taps */
    /* ---- cube scoring (searchToMatch, :91-151) ---- */
    int32_t ncell;           /* int(searchRadius/step): cube is [ntheta][2*ncell+1][2*ncell+1] */
    int32_t ntheta;
    int32_t fine;            /* 1: priors are zero (fineSearch=True) */
    int32_t kmax;            /* capacity of a per-theta cell list (>= beams) */
    const double* thetas;    /* [ntheta] thetaRange (:114) */
    const double* theta_cos; /* [ntheta] np.cos(thetaRange) */
    const double* theta_sin; /* [ntheta] */
    double rv_coef;          /* -(1 / (2 * moveRSigma**2))  (:101) */
    double tw_coef;          /* -1 / (2 * turnSigma**2)     (:108) */
    double max_move_dev;     /* maxMoveDeviation            (:103) */
    /* ---- workspaces, all device, sized for P particles ---- */
    Slam2dFrame* frames;     /* [P] */
    int32_t* axis_x;         /* [P][wmax] field column of every window map column */
    int32_t* axis_y;         /* [P][wmax] */
    uint8_t* occ;            /* [P][fmax][fpitch] occupied field cells; then [P][2 tmax][fp] block flags (8 x 8 cells), fp = (2 tmax + 17) & ~15 */
    uint32_t* field;         /* [P][fmax][fpitch]  fixed-point cost of probSP (see above) */
    int32_t* cells;          /* [P][ntheta][kmax] unique endpoint cells (patch-corner offsets) */
    int32_t* kcount;         /* [P][ntheta] */
    double*  prior;          /* [P][2][ny][nx]  rv plane, thetaWeight plane */
    double*  cube;           /* [P][ntheta][ny][nx] convTotal */
    Slam2dPartial* partials; /* [P][npartial] per-wave reductions of the cube (sweep -> select) */
    int32_t npartial;        /* capacity per particle: ntheta * ceil(ny*nx / 64) */
    int32_t tmax;            /* ceil(fmax / 16): 16x16-cell tiles per field edge */
    uint8_t* tilemask;       /* [P][2 tmax][fp], fp = (2 tmax + 17) & ~15 (the bytes beyond 2 tmax of a row are never written): the 8 x 8-cell block holds an occupied field cell (stamped like occ; must follow
                                occ contiguously: one memset clears both when occ_gen == 0).  Four flags per blur tile: at a blur
                                radius of 8 a tile's halo is exactly its 4 x 4 blocks, so the triage lists exactly the tiles whose
                                halo holds a wall */
    uint8_t* tilestate;      /* [P][tmax][tmax] PERSISTENT across calls: 0 = the field tile already holds
                                the free-space constant (no rewrite needed), 1 = dirty/unknown.
                                Initialise to 1; set to 1 whenever the field buffer is written by
                                anything other than slam2d_field_build */
    double*  tilemin;        /* [P][tmax][tmax] scratch: per-tile minimum of the blurred field */
    double*  tilemax;        /* [P][tmax][tmax] scratch: per-tile maximum of the field as stored */
    int32_t* tilelist;       /* [P][2][tmax*tmax] scratch: work lists (tiles to blur, tiles to fill) */
    int32_t* tilecount;      /* [P][2] scratch: their lengths */
    uint32_t* tileneed;      /* [P][ceil(ntheta/ep_group)][ceil(tmax*tmax/32)] scratch of slam2d_match: bit t of slice (p, g) set
                                = the poses of that group of angles read field tile t; every call rewrites every word, the field build
                                ORs the slices of a particle (may be NULL when only slam2d_field_build is used) */
    unsigned long long* freerow; /* [P][64] scratch (used when tmax <= 64): bit tx of word ty = field tile (ty, tx)
                                holds the free-space constant; lets the sweep skip loads.  NULL disables */
    int32_t* ring;           /* [1 + ring_cap] scratch of SLAM2D_MATCH_PRUNE_BY_PRIOR: length, then the ascending
                                sweep slots (4 consecutive dx of one dy) that hold a pose inside the prior's ring;
                                NULL disables the option */
    int32_t* prune_state;    /* [P] scratch of the same option: 1 = particle needs the full sweep */
    int32_t ring_cap;        /* capacity of ring (ny * ceil(nx / 4) always suffices) */
    /* ---- branch and bound over 4x4 pose tiles (slam2d_match with bnb != 0; see "Branch and bound" below) ---- */
    uint32_t* gmin;          /* [P][4*tmax][4*tmax] minimum cost of every ALIGNED 4x4 block of field cells; written with the
                                field tiles (k_blur_clamp, the triage's constant fill), so it shares tilestate */
    uint32_t* gmin2;         /* [P][4*tmax][4*tmax] element [Y][X] = min(gmin[Y..Y+1][X..X+1]) >> 12: a lower bound of the
                                cost of every field cell in rows 4Y..4Y+7, columns 4X..4X+7 -- whatever 4x4 window starts in
                                block (Y, X) lies inside.  20-bit values: a sum over <= 2048 cells fits 32 bits */
    int32_t* pcells;         /* [P][ntheta][kmax] the endpoint cells again, as byte offsets into a particle's gmin2 */
    double*  bounds;         /* [P][ntheta][nb][4*ceil(nb/4)] upper bound of the score of every pose tile, nb = ceil(nx/4) */
    double*  tile_pmax;      /* [P][nb][4*ceil(nb/4)] largest rv + thetaWeight of a pose tile (+inf if one is NaN) */
    unsigned long long* bnb_best; /* [P] order-preserving bits of the best exact score of the seed tiles */
    /* two-level bounds (bnb == 2: long cell lists): */
    uint32_t* gmin3d;        /* [P][4][2*tmax][2*tmax] min(gmin[Y..Y+2][X..X+2]) >> 12, decimated by two in four phase planes
                                (plane (Y & 1) * 2 + (X & 1), element [Y >> 1][X >> 1]): bounds a tile of 8 x 8 poses */
    int32_t* p3cells;        /* [P][ntheta][kmax] the endpoint cells as byte offsets into a particle's gmin3d */
    double*  bounds1;        /* [P][ntheta][8][8] upper bounds of the 8 x 8-pose tiles */
    unsigned long long* seed_key; /* [P] best finite 8 x 8-tile bound of the particle, packed with its (theta, tile): the seed */
    double*  beam_xy;        /* [P][beams][2] scratch of slam2d_match (may be NULL): beam endpoints of the pose estimate
                                (covertMeasureToXY, Utils/ScanMatcher_OGBased.py:81-89), evaluated once per particle */
    uint32_t* sync;          /* [P][SLAM2D_SYNC_WORDS] arrival counters of the launches whose last-arriving block of a particle
                                finishes the particle's work (k_exact_select split over several blocks; the tile triage as the tail of the
                                scatter).  ZERO them once after allocation; every launch leaves them zero again.  NULL: those
                                launches fall back to one block per particle / separate launches */
    int32_t bnb;             /* 1: slam2d_match scores this level by branch and bound; 2: with two-level bounds; 3: angle bounds
                                (cubes of <= 5 x 5 poses per angle: needs gmin, gmin2, pcells, bounds [P][ntheta], bnb_best, seed_key) */
    int32_t ep_group;        /* angles per k_endpoints block (>= 1; 0 = 1): tileneed holds ceil(ntheta / ep_group) slices per particle */
    int32_t occ_gen;         /* 0: occ + tilemask are cleared at every build.  1..255: generation stamp -- an
                                occ / tilemask byte means "occupied" only when it equals occ_gen, so nothing is
                                cleared; the caller passes a value unused since the buffers were last zeroed
                                (count 1, 2, ... 254, zero the buffers, start again at 1) */
    uint32_t* arrive;        /* NULL, or a device word the wave that writes a particle's Slam2dMatch adds 1 to behind it (ABI 16):
                                slam2d_groups_match sets it on its own copy of a scan's last level (Slam2dScan.match_seq) */
    uint8_t* gmin2b;         /* NULL, or [P][4*tmax][g2b_pitch] (ABI 17): gmin2 >> 12 in bytes (cost >> 24), written beside gmin2.  With it
                                (bnb == 1) the tile bounds of a particle are taken by ONE block that stages this image in LDS
                                (k_bound_lds: 2 LDS cycles per gather instead of ~20 L1 tag lookups); the bounds are looser by
                                < 2^-7 per cell, so a few more tiles are scored exactly -- results unchanged */
    int32_t g2b_pitch;       /* row pitch of gmin2b in bytes: a multiple of 16, >= 4*tmax, (g2b_pitch / 4) mod 32 in [5, 13] or
                                [19, 27] (the tile rows of a lane group then fall on distinct LDS banks) */
    int32_t reserved0;
    double* theta_umax;      /* NULL, or [P][ntheta] (ABI 17, bnb == 1): the largest tile bound of every angle, written with `bounds` by k_bound /
                                k_bound_lds; k_exact_select then reads the bounds only of angles that can hold a surviving tile
                                (theta_umax >= bnb_best - margin): same list, a fraction of the loads */
} Slam2dLevel;

/* Result of one level for one particle. */
typedef struct {
    double x, y, theta;      /* matchedReading pose (:142-143) */
    double confidence;       /* sum(exp(convTotal)) (:141); 0 when it underflows */
    double log_confidence;   /* log of the same, finite when confidence underflows */
    double best_score;       /* max(convTotal) */
    int32_t pick;            /* flat cube index chosen (argmax or soft-max draw) */
    int32_t argmax;          /* flat cube index of the maximum (lowest index on ties) */
} Slam2dMatch;


/* ABI 18: where a beam of a batch of scans writes (slam2d_map_scans), planned by the host as the reference's per-beam growth
 * (Utils/OccupancyGrid.py:144-152) replays: the beam's indices are taken against (lim_x0, lim_y0), the limits after the
 * earlier beams' and scans' growth and before the beam's own; they wrap (a negative index + cols / rows, as Python) against
 * the shape right after the beam's own growth; every low-side growth later in the batch moves them by (ac, ar). */
typedef struct {
    double  lim_x0, lim_y0;  /* mapXLim[0], mapYLim[0] when the beam's indices are computed (:144-145) */
    int32_t dc, dr;          /* low-side shift of the beam's own growth (bookkeeping; the kernel does not read it) */
    int32_t ac, ar;          /* sum of the low-side shifts of every LATER growth of the batch */
    int32_t cols, rows;      /* map shape right after the beam's own growth */
} Slam2dBeamPlan;

/* ------------------------------------------------------------------------- */

int slam2d_abi_version(void);
/* sizeof() of the PODs above as compiled, so the binding can verify its mirror. */
int slam2d_sizeof(const char* type_name);
/* number of visible HIP devices (<= 0: none); never raises. */
int slam2d_device_count(void);

/* frameSearchSpace + generateProbSearchSpace for P particles
 * (Utils/ScanMatcher_OGBased.py:20-45).
 *   d_centre[p*centre_stride + 0..1] = (estimatedX, estimatedY) of particle p.
 * Writes level->frames[p] and level->field[p].  The window must already lie inside
 * each map (the caller performs checkAndExapndOG growth, :27); otherwise
 * SLAM2D_F_WINDOW_OUTSIDE_MAP is raised and the window is clipped. */
int slam2d_field_build(const Slam2dLidar* lidar, const Slam2dLevel* level, const Slam2dMap* d_maps,
                       int32_t P, const double* d_centre, int32_t centre_stride,
                       uint32_t* d_flags, void* stream);

/* searchToMatch for P particles (Utils/ScanMatcher_OGBased.py:91-151).
 *   d_est[p*est_stride + 0..2] = (estimatedX, estimatedY, estimatedTheta)
 *   d_ranges[beams]            = rMeasure (shared by all particles)
 *   est_moving_dist            = estMovingDist
 *   d_psi_cs[P][2]             = (math.cos, math.sin) of estMovingTheta, NaN pair for None
 *                                (NULL: None for every particle; ignored when level->fine)
 *   d_uniform[P]               = one uniform in [0,1) per particle for the soft-max draw
 *                                (matchMax=False, :136-139); NULL selects argmax (matchMax=True)
 * Writes level->cube[p] (convTotal), level->partials[p] and d_out[p]. */
int slam2d_sweep(const Slam2dLidar* lidar, const Slam2dLevel* level, int32_t P,
                 const double* d_est, int32_t est_stride, const double* d_ranges,
                 double est_moving_dist, const double* d_psi_cs, const double* d_uniform,
                 Slam2dMatch* d_out, uint32_t* d_flags, void* stream);

/* matchScan's work at ONE level for P particles: frameSearchSpace + generateProbSearchSpace +
 * searchToMatch (Utils/ScanMatcher_OGBased.py:20-45,91-151) in one call, arguments as for the two
 * calls above (the field is centred on d_est[p][0..1]).  Results (d_out, level->cube,
 * level->partials) are identical to slam2d_field_build followed by slam2d_sweep; the difference is
 * that only the 16x16 field tiles the sweep reads -- those within the search radius of a beam
 * endpoint at some theta -- are blurred (typically 15-30 % of the tiles that hold a wall), so
 * level->field is left incomplete: tiles outside that set keep stale content.  Falls back to the
 * full build for a frame without a single free tile (the field minimum, :43, is then not known
 * without computing everything).
 *
 * options: SLAM2D_MATCH_PRUNE_BY_PRIOR (coarse level only; ignored otherwise).  The reference adds
 * rv = -100 to every pose whose distance from the estimate is not within maxMoveDeviation of the odometry
 * step (:102-103), and no other term of a score is positive.  With this option the poses inside that ring
 * are scored first; when the best of them exceeds -100 + K * max(field) (K = fewest endpoint cells of any
 * theta: the best any pose outside could reach) by SLAM2D_PRUNE_MARGIN, the poses outside cannot be the
 * arg-max and change confidence and soft-max draw by < 1e-12 relative, so they are not scored and
 * level->cube holds only the ring.  Any particle the ring does not settle (best ring score too low, a NaN
 * prior outside the ring) is swept in full by the same call: d_out never differs in arg-max from the
 * unpruned result. */
#define SLAM2D_MATCH_PRUNE_BY_PRIOR 1u
#define SLAM2D_MATCH_PRIOR_READY    2u   /* slam2d_scan_match, slam2d_groups_match[_begin]: d_est / d_psi_cs (the groups: and d_pull) already hold
                                              this scan's prior (slam2d_scan_commit_next, Slam2dScan.h_next_ranges) */
#define SLAM2D_PRUNE_MARGIN 40.0
#define SLAM2D_BNB_MARGIN 30.0
/* Branch and bound (Slam2dLevel.bnb != 0; every level whose cube has 2*ncell+1 in [9, 64] may use it).
 * The cube is cut into tiles of 4 x 4 poses (dy, dx) of one theta.  The poses of a tile read, at endpoint cell k,
 * a 4 x 4 window of the field; that window lies inside the 8 x 8 block of cells gmin2 summarises, so no pose of
 * the tile can score more than
 *     U = -(sum_k gmin2[block of cell k's window] << 12) / cost_scale + max(rv + thetaWeight over the tile).
 * One launch computes U for every tile -- 1/16 of the brute-force gathers, from an image 1/16 the size of the
 * field -- and scores exactly, per theta, the tile with the largest U; the best of those exact scores, M0, is a
 * lower bound of the cube's maximum.  A second launch scores exactly every tile with U >= M0 -
 * SLAM2D_BNB_MARGIN (a fraction of a per cent to a few per cent of the tiles) and selects the pose.  A pose that is
 * skipped scores < max - 30: it cannot be the arg-max, and all skipped poses together (<= 2.4e5 of them at the
 * largest configuration) change confidence and the soft-max draw by < 2.4e5 * exp(-30) = 2.2e-8 relative -- the bar
 * is 1e-5.  A tile holding a NaN prior is always scored (np.argmax returns the first NaN).  level->cube
 * then holds only the scored tiles.
 * bnb == 2 (long cell lists, ~1000 beams): the bounds come in two levels.  Tiles of 8 x 8 poses are bounded first
 * through gmin3d (their 8 x 8 cell window lies inside 3 x 3 aligned 4 x 4 blocks); one exact seed per particle (the
 * best child of the tile with the best 8 x 8 bound, seed_key) gives a first threshold; the 4 x 4 children of the
 * 8 x 8 tiles that reach it get their gmin2 bounds (all other 4 x 4 tiles: -inf), and every theta whose best child
 * still reaches the running maximum is seeded exactly and raises it.  The maximum over all candidate seeds and the
 * tile set scored exactly do not depend on the order in which the waves run.
 * bnb == 3 (angle bounds; cubes of <= 5 x 5 poses per angle, e.g. the fine level behind a coarse factor of 2, with ~1000-cell
 * lists): all poses of one angle read, at endpoint cell k, a window of <= 5 x 5 field cells starting at the patch corner, which
 * lies inside the aligned 8 x 8 block gmin2 summarises there -- so U(theta) = -(sum_k gmin2[cell k] << 12) / cost_scale + the
 * largest prior bounds the angle's whole plane from ONE 4-byte load per cell.  The plane of the particle's best-bound angle is
 * scored exactly first (the seed, M0); planes with U < M0 - SLAM2D_BNB_MARGIN are not scored (level->cube keeps stale content
 * there, their partial reads "nothing"): none of them can hold the arg-max, together they change the confidence by
 * < ntheta * 25 * exp(-30) relative. */
int slam2d_match(const Slam2dLidar* lidar, const Slam2dLevel* level, const Slam2dMap* d_maps, int32_t P,
                 const double* d_est, int32_t est_stride, const double* d_ranges,
                 double est_moving_dist, const double* d_psi_cs, const double* d_uniform,
                 Slam2dMatch* d_out, uint32_t* d_flags, uint32_t options, void* stream);

/* Pose mean and covariance of a match over the WHOLE cube, in one pass (an added symbol: no struct and no existing signature
 * changed, the ABI number stays).  Every pose (it, iy, ix) of the level's cube is scored again, exactly:
 *     s = (-((double)sum_k field[cells[k] + iy*fpitch + ix] * (1/cost_scale)) + rv[iy][ix]) + tw[iy][ix]
 * -- slam2d_sweep's expression over a 64-bit integer sum; an offset outside the particle's field reads 0 and never faults --
 * weighted by w = exp(s - M), M = d_match[p].best_score, and reduced on the fly to the weighted first and second moments of the
 * pose offsets (dx, dy, dtheta) = ((ix - ncell) * step, (iy - ncell) * step, thetas[it]).  level->cube is neither read nor
 * written: after branch and bound it holds only the scored tiles, and what the skipped poses weigh (negligible for the
 * confidence) is multiplied by offsets^2 of up to ncell^2 cells in a second moment.  The sums are taken about the arg-max pose
 * (d_match[p].argmax) and shifted to the mean at the end; no floating-point atomics, a fixed order of summation: the same
 * inputs give the same bits on every call, whichever path of slam2d_match produced them.
 *
 * PRECONDITION.  slam2d_match with any `options`, or slam2d_field_build followed by slam2d_sweep, has run for these P
 * particles on `level`; nothing has written the level's workspaces since; this call is enqueued on the same stream or ordered
 * after that work; d_match is that call's d_out and d_est the estimate it was given (d_est is not read on the device today: the
 * offsets are relative to it).  What the call reads is then complete: level->cells / level->kcount (the unique endpoint cells
 * of every angle, written by every path), level->prior (both planes at both levels; zeros at a fine level), level->thetas and
 * level->field -- slam2d_match builds only the field tiles that the endpoint kernel marks in tileneed, but that kernel marks
 * the tiles of every cell's WHOLE (2*ncell+1)^2 patch, i.e. every field cell some pose of the cube reads, whatever
 * SLAM2D_MATCH_PRUNE_BY_PRIOR or the branch and bound then choose to score (a needed tile that holds the free-space constant
 * holds it in the field, too).  The 16-byte load of the last slot of a pose row may touch cells beyond the patch; those lanes'
 * values are discarded.
 *
 *   d_work: slam2d_match_moments_work(level, P) doubles of scratch
 *           = P * ntheta * ceil((2*ncell+1) * ceil((2*ncell+1) / 4) / 64) * 12 (no HIP call; < 0: SLAM2D_E_*)
 *   d_out[p*SLAM2D_MOMENTS_STRIDE + ...]:
 *      0      sum of w
 *      1-3    mean offset from the estimate (m, m, rad): the mean pose is d_est[p] + mean
 *      4-9    covariance about the mean, normalised by sum w: xx, xy, xtheta, yy, ytheta, thetatheta (world axes)
 *      10     M as used
 *      11     number of poses summed (ntheta * (2*ncell+1)^2)
 *      12     number of NaN scores (a NaN heading prior, Utils/ScanMatcher_OGBased.py:107); > 0: slots 0-9 are NaN
 *      13-15  0
 * No fault bit is raised: the call reads the level and writes only d_work and d_out.  SLAM2D_E_BADARG, before any HIP call:
 * a NULL pointer, P <= 0, est_stride < 3, a level without field, cells, kcount, prior or thetas. */
#define SLAM2D_MOMENTS_STRIDE 16
int slam2d_match_moments(const Slam2dLevel* level, int32_t P, const double* d_est, int32_t est_stride,
                         const Slam2dMatch* d_match, double* d_work, double* d_out, void* stream);
int64_t slam2d_match_moments_work(const Slam2dLevel* level, int32_t P);

/* updateOccupancyGrid for P particles (Utils/OccupancyGrid.py:127-159): one wave per beam walks
 * the cells of the beam's spoke up to the measured range (each window cell belongs to exactly
 * one spoke, each spoke to at most one beam, so the counts are updated without atomics).
 *   d_pose[p*pose_stride + 0..2] = matched (x, y, theta)
 *   d_beam_shift: NULL, or [P][beams][6] int32 reproducing the reference's stale-index writes when the map
 *                 grew during a beam (Utils/OccupancyGrid.py:144-152): (dc, dr) low-side shift of the beam's own
 *                 growth, (ac, ar) sum of the low-side shifts of the later beams, (cols, rows) map shape right
 *                 after the beam's growth; a cell with final index (mx, my) is written at
 *                 wrap(mx - dc - ac, cols) + ac (wrap: a negative index + cols, as Python).  Such writes can land
 *                 on cells of other beams (the reference adds both increments): with d_beam_shift the counts are
 *                 updated atomically and occ_bits is NOT maintained -- call slam2d_map_refresh_bits afterwards.
 * A particle whose pose puts two adjacent window columns or rows on ONE map index (a pose on a half cell of its map) is
 * not updated at all and receives SLAM2D_F_UPDATE_CELL_COLLISION (here and in slam2d_grid_update_weights*, slam2d_scan_commit*,
 * slam2d_groups_commit): the one-writer premise fails there; slam2d_map_scans is exact at such poses.
 * A cell whose map-index quotient ((x + lut_xs[j]) - lim_x0) / unit (or its y twin) is NaN -- a non-finite x or y -- or not below
 * 1e9 in magnitude never reaches a conversion to an integer: it is outside the map, raises SLAM2D_F_UPDATE_OUTSIDE_MAP and
 * writes nothing, with d_beam_shift too.
 * SLAM2D_E_BADARG, before any HIP call, for a lidar no spoke walk can read (also slam2d_occ_extent, slam2d_map_scans,
 * slam2d_predict_scan): NULL, a NULL spoke_band, spoke_cells or spoke_r, num_bands < 1, num_spokes < 1, lut_w < 2 or > 65535,
 * !(unit > 0), or no window coordinates -- lut_xs NULL with lut_xs_step == 0; slam2d_occ_extent and slam2d_map_scans read the
 * table itself and refuse every NULL lut_xs. */
int slam2d_grid_update(const Slam2dLidar* lidar, const Slam2dMap* d_maps, int32_t P,
                       const double* d_pose, int32_t pose_stride, const double* d_ranges,
                       const int32_t* d_beam_shift, uint32_t* d_flags, void* stream);

/* ABI 18: the exact fp64 extent of the occupied points of every (scan, beam) of S scans (Utils/OccupancyGrid.py:142-147:
 * x + xAtSpokeDir[occupiedIdx], y + yAtSpokeDir[occupiedIdx]), the only thing checkMapToExpand (:108-118) asks of them:
 *   d_pose[s*pose_stride + 0..2] = (x, y, theta), d_ranges [S][beams]
 *   d_out [S][beams][4] = (min x, max x, min y, max y); +inf, -inf, +inf, -inf for a beam without occupied cells. */
int slam2d_occ_extent(const Slam2dLidar* lidar, int32_t S, const double* d_pose, int32_t pose_stride, const double* d_ranges,
                      double* d_out, void* stream);

/* ABI 18: updateOccupancyGrid (Utils/OccupancyGrid.py:127-152) for S scans at given poses into ONE map, in one launch, with the
 * reference's semantics exactly -- also where slam2d_grid_update's plain read-modify-write is not: a pose on a half cell (two
 * adjacent window columns or rows round to one map index), a window step that is not the map unit, stale indices that wrap.
 *   d_map:     one map descriptor (device), already grown to the batch's final extent (the host replays the growth from
 *              slam2d_occ_extent and allocates once)
 *   d_plan:    [S][beams] Slam2dBeamPlan
 *   d_lut_bin: [W][W] uint16 spoke bin of every window cell, d_lut_r: [W][W] its radius (spokesGrid, :32-45)
 * A fancy-index statement -- one beam's empty cells (total += 1), its occupied cells (visited += 2, total += 2) -- adds to
 * every map element it names ONCE however many of its cells name it; statements, beams and scans add up (integer atomics: the
 * result does not depend on timing).  Per scan a map element receives at most 3 (1 + 2) from each beam that reaches it; when the
 * scan's window lies inside the map (no growth, no wrap) at most four window cells reach one element, so at most 8.  A narrow
 * map raises SLAM2D_F_COUNT_OVERFLOW if a `total` passed 16 bits (the host promotes before that can happen); a cell outside
 * the map (the reference: IndexError) raises SLAM2D_F_UPDATE_OUTSIDE_MAP and is skipped.  d_flags[0] receives the bits.
 * occ_bits is NOT maintained: call slam2d_map_refresh_bits afterwards. */
int slam2d_map_scans(const Slam2dLidar* lidar, const Slam2dMap* d_map, int32_t S, const double* d_pose, int32_t pose_stride,
                     const double* d_ranges, const Slam2dBeamPlan* d_plan, const uint16_t* d_lut_bin, const double* d_lut_r,
                     uint32_t* d_flags, void* stream);

/* The scan a map expects at a pose, per beam: the inverse of updateOccupancyGrid in the update's own discretisation (an added
 * symbol: no struct and no existing signature changed, the ABI number stays).  The update writes a beam's wall into the cells of ONE
 * angular spoke of the window (Utils/OccupancyGrid.py:131-152), so the range a map predicts for the beam is the nearest occupied
 * cell of that spoke -- a map predicts back exactly the walls the update put there.  For pose s = (x, y, theta) in map
 * d_maps[s * map_stride] (map_stride 1: one map per pose, the filter's P particles in P maps; 0: every pose in map 0) and beam b:
 *   1. spoke = (spoke_start + (int)rint(theta / (2 pi) * num_spokes) + b) mod num_spokes, in [0, num_spokes): the heading is
 *      quantised to the angular step, as in the update (:131,134);
 *   2. every cell k of that spoke, window row i, column j, radius r_k = spoke_r[k], has the map index
 *      mx = rint(((x + lut_xs[j]) - lim_x0) / unit), my = rint(((y + lut_xs[i]) - lim_y0) / unit)  (convertRealXYToMapIdx,
 *      :104-105,144-145; computed by the update's own code, whose shortcuts give these integers);
 *   3. cell k is a HIT iff 0 <= mx < cols, 0 <= my < rows, bit (mx & 31) of occ_bits[my * bits_pitch + (mx >> 5)] is set and
 *      r_min < r_k < r_max (both strict).  A cell outside the map is free: no access leaves the map.  A pose with a non-finite
 *      component, or whose quotient theta / (2 pi) * num_spokes or map-index quotient at a window edge (lut_xs = -+max_range) is
 *      not below 1e9 in magnitude, has no hit on any beam and never reaches a conversion to an integer;
 *   4. r_hit = min r_k over the hits; the WALL is the set of hits with r_k < r_hit + (wall_half + wall_half); r_far = max r_k
 *      over the wall, n_hit = the number of cells in the wall.  No hit: r_hit = +inf, r_far = -inf, n_hit = 0;
 *   5. d_out[(s * beams + b) * SLAM2D_PREDICT_STRIDE + 0..3] = r_hit, r_far, (double)n_hit, 0.
 * A min, a max and a count of tabulated radii: the same inputs give the same bits on every call.
 * PRECONDITION: occ_bits is in step with `cells` (the field build's precondition: slam2d_grid_update keeps it, after any other
 * write to `cells` call slam2d_map_refresh_bits).  Unobserved and free cells are not told apart (that needs the counts).
 * No fault bit is raised: the call reads the map descriptors, the bits and the lidar tables, writes only d_out, allocates nothing,
 * enqueues on `stream` and does not synchronise.  SLAM2D_E_BADARG, before any HIP call: a NULL lidar, d_maps, d_pose or d_out, NULL
 * spoke tables, S <= 0, pose_stride < 3, map_stride not 0 or 1, beams <= 0 or > SLAM2D_MAX_BEAMS, !(r_min >= 0), !(r_max > r_min);
 * SLAM2D_E_TOOLARGE: S * ceil(beams / 4) blocks exceed a grid. */
#define SLAM2D_PREDICT_STRIDE 4
int slam2d_predict_scan(const Slam2dLidar* lidar, const Slam2dMap* d_maps, int32_t map_stride, int32_t S,
                        const double* d_pose, int32_t pose_stride, double r_min, double r_max,
                        double* d_out, void* stream);

/* A scan's score at any poses in a level's field: what the sweep sums for ONE pose of a cube, for N free poses anywhere in the
 * frame -- the measurement model of Monte-Carlo localisation (an added symbol: no struct and no existing signature changed, the
 * ABI number stays).  PRECONDITION: slam2d_field_build -- the FULL build; slam2d_match's lazy build leaves stale tiles -- has run
 * for slot p_field of `level` on this stream (or the call is ordered behind it), and nothing has written that slot's field or
 * frame since.  Read: level->frames[p_field] (xlo, ylo, fh, fw), that slot of level->field, fmax, fpitch, step, cost_scale; of
 * `lidar` only beams, fov, max_range.  For pose n = (x, y, theta) at d_pose[n * pose_stride + 0..2] and its scan at
 * d_ranges + n * ranges_stride (ranges_stride 0: one scan for all poses; >= beams: a scan per pose), with B = beams:
 *   1. beam angle, as numpy.linspace(theta - fov/2, theta + fov/2, B) (Utils/ScanMatcher_OGBased.py:82-83): a0 = theta - fov/2,
 *      a1 = theta + fov/2, astep = (a1 - a0) / (B - 1), a_b = (b == B - 1) ? a1 : b * astep + a0; B == 1: a0;
 *   2. beam b is IN RANGE iff r_b < max_range (:84): NaN and +inf are out, 0 and negative ranges are in;
 *   3. in range: px = x + cos(a_b) * r_b, py = y + sin(a_b) * r_b (:87-88), qx = (px - xlo) / step, qy = (py - ylo) / step
 *      (:174-175), in those operations and that order (no contraction);
 *   4. the beam is INSIDE iff |qx| < 1e9 and |qy| < 1e9 (a NaN fails) and cx = (int)qx, cy = (int)qy (truncation, astype(int))
 *      satisfy 0 <= cx < fw, 0 <= cy < fh.  A quotient that fails the guard never reaches a conversion to an integer, and no
 *      field access leaves [0, fh) x [0, fw);
 *   5. U = the SET of cells (cy, cx) of the inside beams (np.unique, :120); sum_u = sum over U of field[cy * fpitch + cx],
 *      sum_b = the same sum over every inside beam, duplicates counted; 64-bit integers (below 2048 * 2^32 < 2^53);
 *   6. d_out[n * SLAM2D_SCORE_STRIDE + 0..7] =
 *        0  -((double)sum_u * (1 / cost_scale))   the reference's score of the scan at the pose: convTotal of a fine search at zero
 *                                                 offset (:129-130), no prior
 *        1  |U|
 *        2  -((double)sum_b * (1 / cost_scale))   the per-beam score: no reward for folding the scan into few cells
 *        3  inside beams        4  beams in range        5  (double)sum_u        6  (double)sum_b        7  0
 * Sums over a set of integers: the same inputs give the same bits on every call, whichever beam claims a cell.  A pose with a
 * non-finite component has no inside beam (zeros in slots 0-3, 5, 6) and never faults.  No fault bit is raised: the call writes
 * only d_out, allocates nothing, is ONE launch on `stream` and does not synchronise.  SLAM2D_E_BADARG, before any HIP call: a NULL
 * lidar, level, d_pose, d_ranges or d_out, a level without field or frames, N <= 0, p_field < 0, pose_stride < 3, ranges_stride
 * neither 0 nor >= beams, beams < 1 or > SLAM2D_MAX_BEAMS, !(max_range > 0), !(step > 0), !(cost_scale > 0), fmax <= 0 or
 * fpitch < fmax; SLAM2D_E_TOOLARGE: the poses exceed one launch (4 poses per 256 threads, 2 per 128 above 1365 beams, fewer than 2^32
 * threads), or fmax * fpitch >= 2^29 (slam2d_field_build's own limit). */
#define SLAM2D_SCORE_STRIDE 8
int slam2d_score_poses(const Slam2dLidar* lidar, const Slam2dLevel* level, int32_t p_field, int32_t N,
                       const double* d_pose, int32_t pose_stride,
                       const double* d_ranges, int32_t ranges_stride,
                       double* d_out, void* stream);

/* A geometric ray in a field's own frame, for any number of free poses, and the first cost built on it: the range a field expects
 * at a pose, per beam (slam2d_cast_rays), and slam2d_search_lattice's cost plus a charge per beam whose measured range lies beyond
 * a wall of the field (slam2d_score_rays) -- the endpoint model charges a beam only where it ends, so a pose on the wrong side of a
 * wall pays nothing for the beams it sends through it (Thrun, Burgard, Fox, Probabilistic Robotics, 6.3-6.4).  Not
 * slam2d_predict_scan, which is the map update's inverse on the sensor's spoke tables (map resolution, heading quantised to a
 * spoke, one wave per beam).  Added symbols: no struct and no existing signature changed, the ABI number stays.
 * Read by both calls: level->frames[p_field] (xlo, ylo, fh, fw), level->step, fmax, fpitch; of `lidar` beams, fov, max_range;
 * d_dist2, the image slam2d_field_build_distance wrote for the same slot and frame: uint32, cell (i, j) of slot p at
 * (p * fmax + i) * fpitch + j.  slam2d_score_rays also reads that slot of level->field.  Nothing else of `lidar` or `level` is read.
 * PRECONDITION: d_dist2 was made with lut_n >= 2 -- then a value of 0 means occupied and nothing else does, and any clamped
 * value v is a lower bound on the true squared distance --, on this stream or ordered in front of the call, and nothing has
 * written the slot's frame since (slam2d_score_rays: nor its field; any FULL build may have made the field, on the same frame).
 * THE RAY of pose n = (x, y, theta) at d_pose[n * pose_stride + 0..2] and beam b: a_b as in step 1 of slam2d_score_poses,
 * c = cos(a_b), s = sin(a_b); sample k = 0, 1, 2, ..., every operation rounded, in this order, no contraction:
 *     t = (double)k * step,  px = x + c * t,  py = y + s * t,  qx = (px - xlo) / step,  qy = (py - ylo) / step
 * A sample is INSIDE iff 0 <= qx < 1e9 and 0 <= qy < 1e9 (a NaN fails) and (int)qx < fw and (int)qy < fh; its cell is
 * ((int)qy, (int)qx).  Note the `0 <=`: a sample with a quotient in (-1, 0) is OUTSIDE, where the endpoint rule of
 * slam2d_score_poses truncates such a quotient into cell 0 -- on purpose: every ray cell is a unit square, which the kernel's
 * skips over provably free samples need.  The ray ENDS at the first sample that is not inside (LEFT at
 * that k) or at the first inside sample whose cell is occupied (HIT at that k); a ray that reaches its limit K with neither is
 * NONE.  A pose with a non-finite component is LEFT at 0.  No access leaves [0, fh) x [0, fw), and no quotient that fails the
 * guard is converted to an integer.  Integer results: the same inputs give the same bits on every call, whatever the clamp of
 * d_dist2 (it changes which samples are examined, never the answer).
 * slam2d_cast_rays: d_out[n * beams + b] = kind << 30 | k, kind SLAM2D_RAY_HIT (0), SLAM2D_RAY_LEFT (1), or SLAM2D_RAY_NONE (2)
 * with k = K + 1; 0 <= K < 2^20.  ONE launch on `stream`, a wave per 64 beams of a pose; no allocation, no fault bit, no
 * synchronisation.  SLAM2D_E_BADARG, before any HIP call: a NULL lidar, level, d_dist2, d_pose or d_out, a level without frames,
 * N <= 0, p_field < 0, pose_stride < 3, K < 0, beams < 1 or > SLAM2D_MAX_BEAMS, !(max_range > 0), !(step > 0), fmax <= 0 or
 * fpitch < fmax; SLAM2D_E_TOOLARGE: K >= 2^20, fmax * fpitch >= 2^29, N * ceil(beams / 64) waves exceed one launch (fewer than
 * 2^32 threads).
 * slam2d_score_rays: for pose n and its scan at d_ranges + n * ranges_stride (0: one scan for all poses; >= beams: a scan per
 * pose), steps 1-4 of slam2d_score_poses give IN RANGE, INSIDE and sum_b exactly as they do there.  A beam in range is CHECKED iff
 * its quotient r_b / step (one true division) lies in [0, 1e9); then kend = (int64)(r_b / step) - margin, margin >= 0, and the
 * beam is THROUGH iff kend >= 0 and its ray is HIT at some k <= kend; depth_b = kend - k_hit of a through beam.
 *     cost = sum_b + (uint64)(in_range - inside) * outside_cost + (uint64)through * through_cost            (below 2^53)
 *     d_out[n * SLAM2D_RAYS_STRIDE + 0..7] = (double)cost, (double)sum_b, inside, in_range, through, checked, sum of depth_b, 0
 * With through_cost == 0 the cost is slam2d_search_lattice's.  ONE launch on `stream`, a wave per pose (slam2d_score_poses'
 * shape); the sums of a pose are joined as integers, no atomic; no allocation, no fault bit, no synchronisation.
 * SLAM2D_E_BADARG, before any HIP call: the cases of slam2d_cast_rays but K's, a level without a field, a NULL d_ranges,
 * ranges_stride neither 0 nor >= beams, margin < 0; SLAM2D_E_TOOLARGE: fmax * fpitch >= 2^29, the poses exceed one launch (4
 * poses per 256 threads, fewer than 2^32 threads). */
#define SLAM2D_RAYS_STRIDE 8
#define SLAM2D_RAY_HIT  0u
#define SLAM2D_RAY_LEFT 1u
#define SLAM2D_RAY_NONE 2u
#define SLAM2D_RAY_MAX_K (1 << 20)
int slam2d_cast_rays(const Slam2dLidar* lidar, const Slam2dLevel* level, int32_t p_field, const uint32_t* d_dist2, int32_t N,
                     const double* d_pose, int32_t pose_stride, int32_t K, uint32_t* d_out, void* stream);
int slam2d_score_rays(const Slam2dLidar* lidar, const Slam2dLevel* level, int32_t p_field, const uint32_t* d_dist2, int32_t N,
                      const double* d_pose, int32_t pose_stride, const double* d_ranges, int32_t ranges_stride,
                      int32_t margin, uint32_t outside_cost, uint32_t through_cost, double* d_out, void* stream);

/* The best heading and its cost at every position of a lattice of poses, for one scan in a level's field: the global search
 * built on slam2d_score_poses' definition, on the device from the lattice's nine numbers to a [ny][nx] image -- no pose is
 * uploaded, nothing is stored per pose (an added symbol: no struct and no existing signature changed, the ABI number stays).
 * PRECONDITION: that of slam2d_score_poses (the FULL slam2d_field_build has run for slot p_field of `level`, ordered in front
 * of this call); the same members of `level` and `lidar` are read.  Lattice pose (it, iy, ix), 0 <= it < nth, 0 <= iy < ny,
 * 0 <= ix < nx:
 *   x = x0 + (double)ix * dx,  y = y0 + (double)iy * dy,  theta = th0 + (double)it * dth
 * each a rounded product, then an add (no contraction: NumPy's x0 + np.arange(nx) * dx has the same bits).  For that pose and
 * the ONE scan d_ranges[beams], steps 1-5 of slam2d_score_poses define sum_b, the number of INSIDE beams and of beams IN RANGE,
 * identical in every operation and their order (the true division (px - xlo) / step and the 1e9 guard included); sum_u and |U|
 * are not computed.
 *   cost(it, iy, ix) = sum_b + (uint64)(in_range - inside) * outside_cost       (below 2^44 at 2048 beams)
 * -- without the second term a pose whose beams leave the field would pay nothing for them and win --
 *   d_out[iy * nx + ix] = (min over it of cost) << 16 | it_min,   it_min the LOWEST heading index that attains the minimum,
 * i.e. the 64-bit minimum of (cost << 16 | it) over it: independent of the order in which headings are visited.
 *   d_work: slam2d_search_lattice_work(lidar, nx, ny, nth) 8-byte words of scratch (the beams' endpoint offsets cos(a) * r,
 *           sin(a) * r per heading: cos / sin are evaluated nth * beams times, not once per pose and beam)
 * The same inputs give the same bits on every call; the caller need not initialise d_out or d_work.  A non-finite x0, y0 or th0
 * leaves no inside beam (cost = in_range * outside_cost, heading 0) and never reaches a conversion to an integer; no field access
 * leaves [0, fh) x [0, fw).  No fault bit is raised and nothing is allocated: the call enqueues two launches on `stream` (the
 * table and the initial d_out; the search, which joins its heading chunks with a 64-bit integer atomicMin on d_out) and does not
 * synchronise.  SLAM2D_E_BADARG, before any HIP call: a NULL lidar, level, d_ranges or d_out, a NULL d_work where the work size
 * is > 0, a level without field or frames, p_field < 0, nx, ny or nth < 1, nth > 65536, a non-finite dx, dy or dth, beams < 1 or
 * > SLAM2D_MAX_BEAMS, !(max_range > 0), !(step > 0), !(cost_scale > 0), fmax <= 0 or fpitch < fmax; SLAM2D_E_TOOLARGE:
 * nx * ny >= 2^31, a work size beyond 2^31 words (2 * nth * beams: at most 2^28 within the limits above), fmax * fpitch >= 2^29.
 * slam2d_search_lattice_work makes no HIP call; < 0 means SLAM2D_E_* (the lidar, nx, ny, nth cases above). */
int slam2d_search_lattice(const Slam2dLidar* lidar, const Slam2dLevel* level, int32_t p_field,
                          int32_t nx, int32_t ny, int32_t nth,
                          double x0, double dx, double y0, double dy, double th0, double dth,
                          const double* d_ranges, uint32_t outside_cost,
                          uint64_t* d_work, uint64_t* d_out, void* stream);
int64_t slam2d_search_lattice_work(const Slam2dLidar* lidar, int32_t nx, int32_t ny, int32_t nth);

/* A local correlative search around each of N free seed poses, all in ONE field, in one call: the scan matcher on the field of
 * slam2d_score_poses -- every seed gets the best pose of a small lattice about it, and the result stays on the device, where the
 * next stage or the next scan starts from it (added symbols: no struct and no existing signature changed, the ABI number stays).
 * PRECONDITION: that of slam2d_score_poses (a FULL build -- slam2d_field_build or slam2d_field_build_distance -- has run for slot
 * p_field of `level`, ordered in front of this call); the same members of `level` and `lidar` are read.  Everything below is an
 * integer operation or ONE rounded IEEE operation at a time (no contraction), so NumPy reproduces it bit for bit.
 *   a. MOVE.  (x, y, th) = d_pose_in[n * pose_stride + 0..2].  With motion = (dfwd, dside, dturn):  c = cos(th), s = sin(th),
 *        xm = (x + c * dfwd) - s * dside,   ym = (y + s * dfwd) + c * dside,   tm = th + dturn
 *      -- step b of slam2d_mcl_step with fx = dfwd, fy = dside and no noise term.  motion == NULL: (xm, ym, tm) = (x, y, th), bit
 *      for bit.
 *   b. CANDIDATES.  nx = 2 rx + 1, ny = 2 ry + 1, nth = 2 rt + 1; an axis index j counts from the centre outwards,
 *        off(j) = ((j + 1) >> 1) * ((j & 1) ? +1 : -1)  =  0, +1, -1, +2, -2, ...
 *      and candidate (jt, jy, jx), 0 <= jt < nth, 0 <= jy < ny, 0 <= jx < nx, is the pose
 *        x' = xm + (double)off(jx) * dx,   y' = ym + (double)off(jy) * dy,   th' = tm + (double)off(jt) * dth
 *      (a rounded product, then an add) with the flat index f = (jt * ny + jy) * nx + jx: f = 0 is the moved seed itself.
 *   c. COST.  For the pose (x', y', th') and the scan at d_ranges + n * ranges_stride (ranges_stride 0: one scan for all seeds;
 *      >= beams: a scan per seed), steps 1-4 of slam2d_score_poses define sum_b, the INSIDE beams and the beams IN RANGE, the true
 *      division, the 1e9 guard and the truncation included;
 *        cost(f) = sum_b + (uint64)(in_range - inside) * outside_cost           (slam2d_search_lattice's cost, below 2^44)
 *   d. RESULT.  d_out[n * SLAM2D_REFINE_STRIDE + 0] = the 64-bit minimum over f of (cost(f) << 20 | f): among equal costs the
 *      candidate nearest the seed in the order of b wins -- a scan without a return leaves the pose where the odometry put it;
 *      the lowest-index rule of slam2d_search_lattice over a signed lattice would push it into a corner on every scan.
 *      d_out[n * SLAM2D_REFINE_STRIDE + 1] = cost(0), the moved seed's own cost.
 *      d_pose_out[n * pose_stride + 0..2] = (x', y', th') of the winning candidate, by the three operations of b (the other
 *      slots of the stride are untouched).
 *   e. A seed with a non-finite component has no inside beam at any candidate: every cost is in_range * outside_cost and f = 0
 *      wins.  No quotient that fails the guard is converted to an integer; no field access leaves [0, fh) x [0, fw).
 * d_pose_in and d_pose_out are different buffers (stages ping-pong between them).  d_work: slam2d_refine_work(N) = 3 * N 8-byte
 * words of scratch (the moved seeds; the join needs none: it is on d_out).  The caller need not initialise d_work, d_out or
 * d_pose_out; the same inputs give the same bits on every call.  The call allocates nothing, raises no fault bit, enqueues three
 * launches on `stream` -- the move, a thread per seed, which also sets d_out's minima to all ones; the search, a block of 256
 * threads per seed and group of headings, which evaluates cos / sin nth * beams times per seed (a table of endpoint offsets per
 * heading in LDS), not once per candidate, and joins with a 64-bit integer atomicMin on d_out; the winning poses, a thread per
 * seed -- and does not synchronise.  Few seeds spread over the card: a seed's headings are split over up to 1024 / N blocks.
 * SLAM2D_E_BADARG, before any HIP call: the level and lidar cases of slam2d_score_poses, a NULL d_pose_in, d_pose_out, d_ranges,
 * d_out or d_work, d_pose_in == d_pose_out, N < 1, pose_stride < 3, ranges_stride neither 0 nor >= beams, rx, ry or rt < 0, a
 * non-finite dx, dy, dth or motion component; SLAM2D_E_TOOLARGE: nx * ny * nth > SLAM2D_REFINE_MAX_CANDIDATES (the product in 64
 * bits), more than SLAM2D_REFINE_MAX_BLOCKS blocks in the search launch -- N * ceil(nth / hc), hc = min(max(1, 2048 / beams),
 * ceil(nth / ceil(1024 / N))) headings per block: N <= 2^23 seeds where nth <= 2048 / beams, N = 2^20 up to eight times that --,
 * fmax * fpitch >= 2^29.  slam2d_refine_work makes no HIP call; < 0 means SLAM2D_E_* (N < 1: BADARG; N >
 * SLAM2D_REFINE_MAX_BLOCKS: TOOLARGE). */
#define SLAM2D_REFINE_STRIDE 2
#define SLAM2D_REFINE_MAX_CANDIDATES (1 << 20)
#define SLAM2D_REFINE_MAX_BLOCKS (1 << 23)
int64_t slam2d_refine_work(int32_t N);
int slam2d_refine_poses(const Slam2dLidar* lidar, const Slam2dLevel* level, int32_t p_field, int32_t N,
                        const double* d_pose_in, double* d_pose_out, int32_t pose_stride,
                        const double* d_ranges, int32_t ranges_stride,
                        const double motion[3],                 /* NULL: none */
                        int32_t rx, int32_t ry, int32_t rt, double dx, double dy, double dth,
                        uint32_t outside_cost, uint64_t* d_work, uint64_t* d_out, void* stream);

/* slam2d_refine_poses with slam2d_score_rays' charge per beam that crosses a wall inside the COST of every candidate, on a stride
 * of the beams: a lattice that straddles a wall no longer steps to the wrong side of it for nothing, which matters most to a
 * tracker of ONE pose, which has no cloud to outvote the mistake (added symbols: no struct and no existing signature changed, the
 * ABI number stays).  PRECONDITION: those of slam2d_refine_poses and of slam2d_score_rays -- d_dist2 is the image
 * slam2d_field_build_distance wrote for slot p_field with lut_n >= 2, on the frame the slot's field was built on.  The same members
 * of `level` and `lidar` are read.  Integer operations and ONE rounded IEEE operation at a time (no contraction): NumPy reproduces
 * it bit for bit and the same inputs give the same bits on every call.
 * Steps a (MOVE), b (CANDIDATES), d (RESULT) and e are slam2d_refine_poses' as written there, and
 *   c. COST.  For candidate f = (x', y', th') and the seed's scan, sum_b, INSIDE and IN RANGE exactly as in slam2d_refine_poses.
 *      Beam b is CAST iff b % ray_stride == ray_phase.  A CAST beam in range is CHECKED iff its quotient r_b / step (one true
 *      division) lies in [0, 1e9); then kend = (int64)(r_b / step) - margin, and the beam is THROUGH iff kend >= 0 and THE RAY
 *      (above slam2d_cast_rays: the same sample formula, the `0 <=` guard, d_dist2) from (x', y') along a_b -- formed from th'
 *      exactly as the endpoint's: a0 = th' - fov/2, ..., c = cos(a_b), s = sin(a_b) -- is HIT at some k <= kend.  through(f) = the
 *      number of THROUGH beams of the candidate;
 *        cost(f) = sum_b + (uint64)(in_range - inside) * outside_cost + (uint64)through(f) * through_cost
 *      -- below 2^44 by the argument of slam2d_mcl_step_rays (two terms of at most 2048 * 2^32 = 2^43), so cost(f) << 20 | f still
 *      fits one 64-bit word.
 *   RESULT.  d_out[n * SLAM2D_REFINE_STRIDE + 0] = the 64-bit minimum over f of (cost(f) << 20 | f) on this cost, word 1 = the
 *      charged cost(0), d_pose_out the winning candidate by the three operations of b.  d_through: NULL (not wanted), or [N]:
 *      d_through[n] = through(f) of the winning candidate.  A seed with a non-finite component keeps f = 0 with through = 0: its
 *      ray is LEFT at 0 on every beam.
 * EQUIVALENCES.  (i) With through_cost == 0, or no CAST beam (ray_phase >= beams), or a margin beyond every range's quotient, the
 * two words and d_pose_out are slam2d_refine_poses' bit for bit.  (ii) With ray_stride == 1, word 0 is the minimum over f of
 * (slot 0 of slam2d_score_rays at the materialised candidate f, same margin and costs, the seed's scan) << 20 | f, word 1 is that
 * call's slot 0 at f = 0, and d_through[n] its slot 4 at the winner.
 * d_work: slam2d_refine_rays_work(N) == slam2d_refine_work(N) words; the caller need not initialise d_work, d_out, d_pose_out or
 * d_through.  The call allocates nothing, raises no fault bit, does not synchronise and enqueues three launches on `stream`: the
 * move, slam2d_refine_poses' own; the search, a block of 256 threads per seed and hc headings -- hc is slam2d_refine_poses': hc =
 * min(max(1, 2048 / beams), ceil(nth / ceil(1024 / N))); the block keeps a second LDS table, the unit vectors (cos a_b, sin a_b)
 * per heading and KEPT beam, beside the endpoint offsets, both from one evaluation of cos / sin: the headings per row stay, the
 * block's LDS grows to 16 hc (beams + J) + 4 (beams + J) bytes, J the number of cast beams, at most 80 KiB --, where
 * the KEPT beams are the cast beams that are CHECKED with kend >= 0 (no other can be THROUGH at any pose), compacted once per
 * block, the lanes of a wave are neighbouring positions of one heading and walk one beam's parallel rays together, and the join
 * is the 64-bit integer atomicMin on d_out; the winners, where d_through is wanted a wave per seed, which recasts the winner's
 * cast beams packed over its lanes by the search's own expressions (d_through == NULL: slam2d_refine_poses' own last launch).
 * Every ray ends: its sample index strictly increases below kend + 1 < 2^30.
 * SLAM2D_E_BADARG, before any HIP call: every case of slam2d_refine_poses, a NULL d_dist2, ray_stride < 1 or > SLAM2D_MAX_BEAMS,
 * ray_phase < 0 or >= ray_stride, margin < 0; SLAM2D_E_TOOLARGE: as there -- nx * ny * nth > SLAM2D_REFINE_MAX_CANDIDATES, more
 * than SLAM2D_REFINE_MAX_BLOCKS blocks in the search launch, N * ceil(nth / hc) with the hc above (the last launch has
 * ceil(N / 4)), fmax * fpitch >= 2^29, a device that does not grant the block its LDS.  slam2d_refine_rays_work makes no HIP call and answers what slam2d_refine_work answers,
 * error codes included. */
int64_t slam2d_refine_rays_work(int32_t N);                     /* slam2d_refine_work(N) */
int slam2d_refine_poses_rays(const Slam2dLidar* lidar, const Slam2dLevel* level, int32_t p_field, const uint32_t* d_dist2, int32_t N,
                             const double* d_pose_in, double* d_pose_out, int32_t pose_stride,
                             const double* d_ranges, int32_t ranges_stride,
                             const double motion[3],            /* NULL: none */
                             int32_t rx, int32_t ry, int32_t rt, double dx, double dy, double dth, uint32_t outside_cost,
                             int32_t ray_stride, int32_t ray_phase, int32_t margin, uint32_t through_cost,
                             uint32_t* d_through,               /* NULL: not wanted */
                             uint64_t* d_work, uint64_t* d_out, void* stream);

/* The two on-device searches for a SET OF POINTS in the robot's frame instead of one scan of one sensor: several scans joined by
 * odometry, two sensors on one robot, a sensor off the robot's origin, a driver's own or de-skewed beam angles -- whatever the
 * caller can express as points (added symbols: no struct and no existing signature changed, the ABI number stays).  The scan
 * forms look at a beam in one place only, the table of endpoint offsets per heading; here that table is R(theta) q, and
 * everything behind it is slam2d_search_lattice's and slam2d_refine_poses'.  PRECONDITION: that of slam2d_score_poses (a FULL
 * build -- slam2d_field_build or slam2d_field_build_distance -- has run for slot p_field of `level`, ordered in front of this
 * call); the same members of `level` are read.  No Slam2dLidar is taken: nothing of one is read.  Everything below is an integer
 * operation or ONE rounded IEEE operation at a time (no contraction), so NumPy reproduces it bit for bit.
 * Point k of a set, 0 <= k < M, is (qx, qy) = d_points[k * point_stride + 0..1] in the robot's frame: x forward, y to the left,
 * metres (the other slots of the stride are not read).  For a pose (x, y, th):
 *   1. point k is VALID iff qx and qy are both finite; invalid points are dropped, as beams out of range are.  valid = their
 *      number: it does not depend on the pose;
 *   2. c = cos(th), s = sin(th);  ex = (c * qx) - (s * qy),  ey = (s * qx) + (c * qy);
 *   3. px = x + ex, py = y + ey, and from there steps 3-4 of slam2d_score_poses as written there: the true division
 *      (px - xlo) / step, the 1e9 guard in front of the conversion, the truncation, 0 <= cx < fw and 0 <= cy < fh; sum_b = the
 *      sum of field[cy * fpitch + cx] over the INSIDE points, duplicates counted;
 *   4. cost = sum_b + (uint64)(valid - inside) * outside_cost                  (below 2^44 at SLAM2D_MAX_POINTS points)
 * A valid point whose rotated offset overflows, or a non-finite pose component, leaves the point not inside: it pays
 * outside_cost.  No quotient that fails the guard reaches a conversion to an integer; no field access leaves [0, fh) x [0, fw).
 * A set without a valid point costs 0 at every pose.
 * slam2d_search_points is slam2d_search_lattice with that cost: the same lattice poses x0 + (double)ix * dx, y0 + (double)iy * dy,
 * th0 + (double)it * dth, the same word d_out[iy * nx + ix] = the 64-bit minimum over it of (cost << 16 | it), the same two
 * launches -- the table E[it][k] = (ex, ey) of the k-th valid point in d_work (slam2d_search_points_work(M, nx, ny, nth) =
 * 2 * nth * M 8-byte words) with the initial all-ones of d_out, a block per heading; then the search with its atomicMin join.
 * cos / sin are evaluated nth times, not nth * M times.
 * slam2d_refine_points is slam2d_refine_poses with that cost: the same MOVE (a), CANDIDATES (b: off(j), the flat index f) and
 * RESULT (d: cost << 20 | f, cost(0) in word 1, the winning pose by the candidates' three operations; e: a seed with a
 * non-finite component keeps f = 0), d_work of slam2d_refine_work(N) words and the same three launches; the search block keeps
 * its table in LDS, at most 2048 / M headings per block row, a seed's headings split over up to 1024 / N blocks.  cos / sin are
 * evaluated once per heading and seed.  set_stride 0: the one set d_points for every seed; set_stride >= M * point_stride
 * doubles: a set per seed, seed n's at d_points + n * set_stride.
 * In both the caller need not initialise d_work, d_out or d_pose_out; the same inputs give the same bits on every call; nothing
 * is allocated, no fault bit is raised, nothing synchronises.  SLAM2D_E_BADARG, before any HIP call: the level cases of
 * slam2d_score_poses (a NULL level, no field or frames, p_field < 0, !(step > 0), !(cost_scale > 0), fmax <= 0 or fpitch <
 * fmax), a NULL d_points, d_out, d_work, d_pose_in or d_pose_out, M < 1 or > SLAM2D_MAX_POINTS, point_stride < 2, set_stride
 * neither 0 nor >= M * point_stride, N < 1, pose_stride < 3, d_pose_in == d_pose_out, rx, ry or rt < 0, nx, ny or nth < 1,
 * nth > 65536, a non-finite dx, dy, dth or motion component; SLAM2D_E_TOOLARGE: nx * ny >= 2^31 (search); nx * ny * nth >
 * SLAM2D_REFINE_MAX_CANDIDATES or more than SLAM2D_REFINE_MAX_BLOCKS blocks -- N * ceil(nth / hc), hc = min(max(1, 2048 / M),
 * ceil(nth / ceil(1024 / N))) -- (refine); fmax * fpitch >= 2^29.  slam2d_search_points_work makes no HIP call; < 0 means
 * SLAM2D_E_* (the M, nx, ny, nth cases above).
 * slam2d_score_points, slam2d_mcl_step_points and slam2d_mcl_step_adaptive_points (below slam2d_mcl_step_adaptive) are the point
 * forms of slam2d_score_poses and of the two MCL steps, on this cost. */
#define SLAM2D_MAX_POINTS SLAM2D_MAX_BEAMS        /* 2048: cost stays below 2^44, one heading fits REFINE_TABLE */
int64_t slam2d_search_points_work(int32_t M, int32_t nx, int32_t ny, int32_t nth);   /* 2 * nth * M words */
int slam2d_search_points(const Slam2dLevel* level, int32_t p_field,
                         int32_t nx, int32_t ny, int32_t nth,
                         double x0, double dx, double y0, double dy, double th0, double dth,
                         const double* d_points, int32_t point_stride, int32_t M,
                         uint32_t outside_cost, uint64_t* d_work, uint64_t* d_out, void* stream);
int slam2d_refine_points(const Slam2dLevel* level, int32_t p_field, int32_t N,
                         const double* d_pose_in, double* d_pose_out, int32_t pose_stride,
                         const double* d_points, int32_t point_stride, int32_t M, int32_t set_stride,
                         const double motion[3],                /* NULL: none */
                         int32_t rx, int32_t ry, int32_t rt, double dx, double dy, double dth,
                         uint32_t outside_cost, uint64_t* d_work, uint64_t* d_out, void* stream);

/* One step of Monte-Carlo localisation in a known map: N pose hypotheses are moved by the odometry increment, weighed against the
 * ONE field of slot p_field with slam2d_score_poses' measurement model, resampled, and left on the device -- no host decision in
 * between (an added symbol: no struct and no existing signature changed, the ABI number stays).  PRECONDITION: that of
 * slam2d_score_poses (the FULL slam2d_field_build has run for slot p_field of `level`, ordered in front of this call); the same
 * members of `level` and `lidar` are read.  Everything below is an integer operation or ONE rounded IEEE operation at a time (no
 * contraction), so NumPy reproduces it bit for bit and the same inputs give the same bits on every call.
 *   a. NOISE.  Philox4x32-10 (Salmon, Moraes, Dror, Shaw 2011): multipliers M0 = 0xD2511F53, M1 = 0xCD9E8D57, key increments
 *      0x9E3779B9, 0xBB67AE85; one round maps the counter c to [hi(M1 * c2) ^ c1 ^ k0, lo(M1 * c2), hi(M0 * c0) ^ c3 ^ k1,
 *      lo(M0 * c0)] and then bumps the key; ten rounds.  Key = (seed low, seed high).  For particle n and draw j in {0, 1, 2} the
 *      counter is (n, j, scan low, scan high); S = the sum of the four output words read as int32, in 64 bits, and
 *      g_j = (double)S * 2^-31: exact, |g| < 4, approximately normal -- the Irwin-Hall sum of four uniforms, variance 4/3, support
 *      +/- 3.46 sigma (no tail beyond).  The resampler's word r is output word 0 of the counter (0xffffffff, 0, scan low, scan high).
 *   b. MOVE.  With (x, y, th) = d_pose_in[n * pose_stride + 0..2], motion = (dfwd, dside, dturn) -- the odometry increment in the
 *      robot's own previous frame -- and amp (noise amplitudes: std = amp * sqrt(4/3); 0 = none), each product and sum rounded,
 *      in this order:  fx = dfwd + amp[0] * g_0,  fy = dside + amp[1] * g_1,  c = cos(th), s = sin(th),
 *        x' = (x + c * fx) - s * fy,   y' = (y + s * fx) + c * fy,   th' = (th + dturn) + amp[2] * g_2.
 *   c. WEIGH.  For the moved pose and the ONE scan d_ranges[beams], steps 1-4 of slam2d_score_poses define sum_b (the field's sum
 *      over every inside beam), the INSIDE beams and the beams IN RANGE, the true division and the 1e9 guard included; no cell set
 *      is built.  cost_n = sum_b + (uint64)(in_range - inside) * outside_cost (slam2d_search_lattice's cost, below 2^44);
 *      cmin = the minimum cost, best = the LOWEST n that attains it (the 64-bit minimum of cost << 20 | n);
 *        w_n = min(d_lut[min((cost_n - cmin) >> lut_shift, lut_n - 1)], SLAM2D_MCL_MAX_WEIGHT)
 *      -- integer weights from a table the host makes (exp(-cost / cost_scale) scaled to 24 bits is the reference's soft-max): no
 *      exp on the device, whose last bit could flip a resampling.
 *   d. RESAMPLE, systematic, in integers.  C_n = the inclusive prefix sum of w, W = C_(N-1) < 2^44;
 *      u0 = floor(r * W / 2^32) = W_hi * r + ((W_lo * r) >> 32);  t_k = floor((k * W + u0) / N) for offspring k (below 2^64, as
 *      w <= 0xffffff and N <= 2^20);  the ancestor a_k = the least n with t_k < C_n;  W == 0: a_k = k.
 *      d_pose_out[k * pose_stride + 0..2] = the moved pose of a_k (the other slots of the stride are untouched);
 *      d_ancestor[k] = a_k where d_ancestor is not NULL.  Ancestors never decrease with k.
 *   e. REPORT.  d_report[0..15], 64-bit words:  0 cmin   1 best   2 W   3 the number of w_n > 0   4 u0   5 in_range
 *      6 the number of DISTINCT ancestors   7-9 the bit patterns of the best particle's moved pose   10 M, the number of offspring
 *      with |x| < 2^20, |y| < 2^20 and a finite th   11-14 the signed sums over those offspring of llrint(x * 65536),
 *      llrint(y * 65536), llrint(cos(th) * 2^30), llrint(sin(th) * 2^30) (two's complement)   15 0.
 *      Sums of integers: x / (65536 M), y / (65536 M) and atan2 of the last two are a mean pose of the same bits on every call.
 *   f. A pose with a non-finite component has no inside beam and costs in_range * outside_cost; no field access leaves
 *      [0, fh) x [0, fw); no quotient that fails the guard is converted to an integer.
 * d_pose_in and d_pose_out are different buffers (ping-pong).  d_work: slam2d_mcl_work(N) 8-byte words of scratch (5 * N + 1032:
 * the moved poses, the costs, the prefix sums).  The caller need not initialise d_work, d_report, d_pose_out or d_ancestor.  The
 * call allocates nothing, raises no fault bit, enqueues five launches on `stream` -- move, a thread per particle; score, a wave
 * per particle, joined by the integer atomicMin; weigh and scan per block of 1024 particles; one block over the at most 1024 block
 * sums; resample -- and does not synchronise: separate launches order the phases, every join is an integer atomic or a fixed
 * prefix sum.  SLAM2D_E_BADARG, before any HIP call: a NULL pointer other than d_ancestor, d_pose_in == d_pose_out, N < 1,
 * pose_stride < 3, lut_n < 1 or > 65536, lut_shift outside 0..43, a non-finite motion or amp, and the level and lidar cases of
 * slam2d_score_poses; SLAM2D_E_TOOLARGE: N > SLAM2D_MCL_MAX_PARTICLES, fmax * fpitch >= 2^29.
 * slam2d_mcl_work makes no HIP call; < 0 means SLAM2D_E_* (N < 1: BADARG; N > SLAM2D_MCL_MAX_PARTICLES: TOOLARGE). */
#define SLAM2D_MCL_REPORT 16
#define SLAM2D_MCL_MAX_PARTICLES (1 << 20)
#define SLAM2D_MCL_MAX_WEIGHT 0xffffffu
int64_t slam2d_mcl_work(int32_t N);
int slam2d_mcl_step(const Slam2dLidar* lidar, const Slam2dLevel* level, int32_t p_field, int32_t N,
                    const double* d_pose_in, double* d_pose_out, int32_t pose_stride,
                    const double motion[3], const double amp[3], uint64_t seed, uint64_t scan,
                    const double* d_ranges, uint32_t outside_cost,
                    const uint32_t* d_lut, int32_t lut_n, int32_t lut_shift,
                    int32_t* d_ancestor, uint64_t* d_work, uint64_t* d_report, void* stream);

/* slam2d_mcl_step with a particle count that lives on the device and follows the spread of the set -- KLD-sampling (Fox 2003)
 * stated in integers: the number of occupied pose bins is the size of a set, the bound a table the host makes, the resampler
 * draws as many offspring as the table says (an added symbol: no existing signature, struct or kernel result changed, the ABI
 * number stays).  n_cap: the capacity, in poses, of BOTH pose buffers, of d_ancestor and of the work arrays (at most
 * SLAM2D_MCL_MAX_PARTICLES).  PRECONDITION and members read: those of slam2d_mcl_step.
 *   LIVE COUNT.  N = min(max(*d_n_in, 1), n_cap), read on the device: the host never needs it.
 *   a-c. NOISE, MOVE, WEIGH: steps a-c of slam2d_mcl_step over the particles n < N -- the same counters (n, j, scan), the same
 *      five rounded operations, the same cost, cmin, best and table weight w_n, the same prefix sums C_n, W, r and u0.  Poses
 *      n >= N of d_pose_in are not read.
 *   d. REFERENCE ANCESTORS.  A = the distinct ancestors of slam2d_mcl_step's resampling with N offspring, t_k =
 *      floor((k * W + u0) / N), k < N: particle n is in A iff some k < N has C_(n-1) * N <= k * W + u0 < C_n * N (products below
 *      2^64, as W <= N * 0xffffff).  W == 0: A = every n < N.
 *   e. BINS of the moved pose (x, y, th) of each member of A:  qx = (x - x0) / cell,  qy = (y - y0) / cell,  qt = th / turn, each
 *      ONE true division.  The pose is BINNABLE when |qx|, |qy| and |qt| are all < 1e9 (a NaN fails) and ix = floor(qx),
 *      iy = floor(qy) satisfy 0 <= ix < nx, 0 <= iy < ny;  it = floor(qt) mod nth, non-negative;  bin = (it * ny + iy) * nx + ix.
 *      Every pose that is not binnable falls into the ONE extra bin n_bins = nx * ny * nth; a quotient that fails the guard is
 *      never converted to an integer.  kbins = the number of distinct bins over A: a bitmap of n_bins + 1 bits set with integer
 *      atomic OR, then a population count.
 *   f. SIZE.  N_out = min(max(d_ntab[min(kbins, ntab_n - 1)], 1), n_cap): a table the host makes (engine.kld_table), no floating
 *      point on the device.
 *   g. RESAMPLE with N_out offspring:  t_j = floor((j * W + u0) / N_out), j < N_out (below 2^64 as before);  a_j = the least n
 *      with t_j < C_n;  W == 0: a_j = j mod N.  d_pose_out[j * pose_stride + 0..2] = the moved pose of a_j; rows j >= N_out are
 *      untouched, and so are the other slots of the stride.  d_ancestor[j] = a_j where d_ancestor is not NULL.  *d_n_out = N_out,
 *      written by the last launch: d_n_in and d_n_out may be the same word.
 *   h. REPORT.  d_report[0..23]:  0-15 are slam2d_mcl_step's -- 0-5 and 7-9 over the N particles, 6 (distinct ancestors) and
 *      10-14 (M and the four sums) over the N_out offspring of step g --,  16 N   17 N_out   18 kbins   19 |A|   20-23 0.
 *   EQUIVALENCE.  With *d_n_in == n_cap and a table that returns n_cap, the first n_cap output poses, d_ancestor and report words
 *   0-15 are slam2d_mcl_step(N = n_cap)'s bit for bit, and word 19 equals word 6.
 * d_work: slam2d_mcl_adapt_work(n_cap, bins) 8-byte words = slam2d_mcl_work(n_cap) + (nx * ny * nth + 64) / 64 (the bitmap) + 8.
 * The caller need not initialise d_work, d_report, d_pose_out or d_ancestor: the call clears the bitmap itself.  It allocates
 * nothing, raises no fault bit and does not synchronise.  Seven launches on `stream` order the phases -- move (and the bitmap's
 * clearing), score, weigh and scan, the block sums, the reference ancestors and their bins, the bitmap's count, the resampling --
 * ; every per-particle launch is a grid of at most a few blocks per compute unit that strides over n < N, so what a call costs
 * follows N and nx * ny * nth / 64, not n_cap.  Every join is an integer atomic or a fixed prefix sum.
 * SLAM2D_E_BADARG, before any HIP call: every case of slam2d_mcl_step (N read as n_cap), a NULL d_n_in, d_n_out, bins or d_ntab,
 * ntab_n < 1 or > 65536, nx, ny or nth < 1, !(cell > 0), !(turn > 0), a non-finite x0 or y0; SLAM2D_E_TOOLARGE: n_cap >
 * SLAM2D_MCL_MAX_PARTICLES, nx * ny * nth > SLAM2D_MCL_MAX_BINS (the product in 64 bits), fmax * fpitch >= 2^29.
 * slam2d_mcl_adapt_work makes no HIP call; < 0 means SLAM2D_E_* (the n_cap and bins cases above). */
typedef struct {            /* pose bins of the KLD count */
    double x0, y0;          /* low corner of the bin window */
    double cell;            /* bin edge, metres (> 0) */
    double turn;            /* bin width, radians (> 0; the host passes 2 pi / nth) */
    int32_t nx, ny, nth, _pad;
} Slam2dMclBins;

#define SLAM2D_MCL_ADAPT_REPORT 24
#define SLAM2D_MCL_MAX_BINS (1 << 26)
int64_t slam2d_mcl_adapt_work(int32_t n_cap, const Slam2dMclBins* bins);
int slam2d_mcl_step_adaptive(const Slam2dLidar* lidar, const Slam2dLevel* level, int32_t p_field, int32_t n_cap,
                             const uint32_t* d_n_in, uint32_t* d_n_out,
                             const double* d_pose_in, double* d_pose_out, int32_t pose_stride,
                             const double motion[3], const double amp[3], uint64_t seed, uint64_t scan,
                             const double* d_ranges, uint32_t outside_cost,
                             const uint32_t* d_lut, int32_t lut_n, int32_t lut_shift,
                             const Slam2dMclBins* bins, const uint32_t* d_ntab, int32_t ntab_n,
                             int32_t* d_ancestor, uint64_t* d_work, uint64_t* d_report, void* stream);

/* slam2d_mcl_step and slam2d_mcl_step_adaptive with slam2d_score_rays' charge per beam that crosses a wall inside the WEIGH step, on
 * a stride of the beams: a cloud on the wrong side of a wall pays for the beams it sends through it and loses the resampling,
 * where the endpoint model lets it live for as many scans as the endpoints alone need (added symbols: no struct and no existing
 * signature changed, the ABI number stays).  PRECONDITION: those of slam2d_mcl_step and of slam2d_score_rays -- d_dist2 is the image
 * slam2d_field_build_distance wrote for slot p_field with lut_n >= 2, on the frame the slot's field was built on.  The same members
 * of `level` and `lidar` are read.  Integer operations and ONE rounded IEEE operation at a time: the same inputs give the same bits
 * on every call.
 * slam2d_mcl_step_rays: steps a (NOISE), b (MOVE), d (RESAMPLE) and e (REPORT) are slam2d_mcl_step's as written there, and
 *   c. WEIGH.  sum_b, INSIDE and IN RANGE of the moved pose exactly as in slam2d_mcl_step.  Beam b is CAST iff
 *      b % ray_stride == ray_phase.  A CAST beam in range is CHECKED iff its quotient r_b / step (one true division) lies in
 *      [0, 1e9); then kend = (int64)(r_b / step) - margin, and the beam is THROUGH iff kend >= 0 and THE RAY (above
 *      slam2d_cast_rays: the same sample formula, the `0 <=` guard, d_dist2) of the moved pose along the beam's own a_b is HIT at
 *      some k <= kend.  through_n = the number of THROUGH beams of particle n;
 *        cost_n = sum_b + (uint64)(in_range - inside) * outside_cost + (uint64)through_n * through_cost
 *      -- below 2^44: sum_b and the outside term together are at most 2048 * 2^32 = 2^43 and so is the through term, so
 *      cost << 20 | n still fits 64 bits.  cmin, best and w_n as in slam2d_mcl_step, on this cost.
 *   REPORT.  Words 0-14 as in slam2d_mcl_step, on this cost; word 15 = the sum of through_n over the N particles, an integer atomic
 *      add, reset with the other joined words by the first launch.
 *   d_through: NULL, or [N]: d_through[n] = through_n of the MOVED particle n, before the resampling.
 * slam2d_mcl_step_adaptive_rays: slam2d_mcl_step_adaptive with that WEIGH step over n < N; its steps d-h are as written there,
 * word 15 is the sum over n < N, d_through is NULL or [n_cap] and its rows n >= N are untouched.
 * EQUIVALENCES.  (i) With through_cost == 0, or no CAST beam (ray_phase >= beams), the output poses, d_ancestor and report words
 * 0-14 are slam2d_mcl_step's (slam2d_mcl_step_adaptive's) bit for bit.  (ii) With ray_stride == 1 and motion = amp = 0, word 0 is
 * the minimum of slam2d_score_rays' cost (same margin and costs, the one scan) over the input poses, word 1 the lowest index that
 * attains it, and d_through equals its slot 4.  (iii) The EQUIVALENCE clause of slam2d_mcl_step_adaptive holds against
 * slam2d_mcl_step_rays, word 15 and d_through included.
 * d_work: slam2d_mcl_rays_work(N) == slam2d_mcl_work(N) words, slam2d_mcl_adapt_rays_work(n_cap, bins) ==
 * slam2d_mcl_adapt_work(n_cap, bins); the caller need not initialise d_work, d_report, d_pose_out, d_ancestor or d_through.  Both
 * calls allocate nothing, raise no fault bit and do not synchronise.  Five launches (adaptive: seven) on `stream`, as in the plain
 * steps: the move launch also resets word 15; the score launch is a wave per particle -- slam2d_mcl_step's endpoint trips, then the
 * CAST beams packed over the wave's lanes, 64 rays per trip (180 beams at stride 4: 45 rays in one trip), through_n joined by
 * ballots, the sixteen particles of a block joined in LDS in front of the block's one integer atomic --; the sums launch leaves word 15 alone; the weigh, reference, count
 * and resample launches are the plain steps' own kernels.  Every ray ends: its sample index strictly increases below kend + 1 < 2^30.
 * SLAM2D_E_BADARG, before any HIP call: every case of slam2d_mcl_step (slam2d_mcl_step_adaptive), a NULL d_dist2, ray_stride < 1
 * or > SLAM2D_MAX_BEAMS, ray_phase < 0 or >= ray_stride, margin < 0; SLAM2D_E_TOOLARGE: as there.  The two *_work functions make no
 * HIP call and answer what slam2d_mcl_work and slam2d_mcl_adapt_work answer, error codes included. */
int64_t slam2d_mcl_rays_work(int32_t N);                        /* slam2d_mcl_work(N) */
int slam2d_mcl_step_rays(const Slam2dLidar* lidar, const Slam2dLevel* level, int32_t p_field, const uint32_t* d_dist2, int32_t N,
                         const double* d_pose_in, double* d_pose_out, int32_t pose_stride,
                         const double motion[3], const double amp[3], uint64_t seed, uint64_t scan,
                         const double* d_ranges, uint32_t outside_cost,
                         int32_t ray_stride, int32_t ray_phase, int32_t margin, uint32_t through_cost,
                         const uint32_t* d_lut, int32_t lut_n, int32_t lut_shift,
                         int32_t* d_ancestor, uint32_t* d_through, uint64_t* d_work, uint64_t* d_report, void* stream);
int64_t slam2d_mcl_adapt_rays_work(int32_t n_cap, const Slam2dMclBins* bins);   /* slam2d_mcl_adapt_work(n_cap, bins) */
int slam2d_mcl_step_adaptive_rays(const Slam2dLidar* lidar, const Slam2dLevel* level, int32_t p_field, const uint32_t* d_dist2,
                                  int32_t n_cap, const uint32_t* d_n_in, uint32_t* d_n_out,
                                  const double* d_pose_in, double* d_pose_out, int32_t pose_stride,
                                  const double motion[3], const double amp[3], uint64_t seed, uint64_t scan,
                                  const double* d_ranges, uint32_t outside_cost,
                                  int32_t ray_stride, int32_t ray_phase, int32_t margin, uint32_t through_cost,
                                  const uint32_t* d_lut, int32_t lut_n, int32_t lut_shift,
                                  const Slam2dMclBins* bins, const uint32_t* d_ntab, int32_t ntab_n,
                                  int32_t* d_ancestor, uint32_t* d_through, uint64_t* d_work, uint64_t* d_report, void* stream);

/* The point forms of slam2d_score_poses, slam2d_mcl_step and slam2d_mcl_step_adaptive: the same calls for a SET OF POINTS in the
 * robot's frame (the comment above SLAM2D_MAX_POINTS: point k at d_points[k * point_stride + 0..1], steps 1-4 of its cost) instead
 * of one scan of one sensor, so that a caller who found a place with slam2d_search_points can grade pose sets and follow the robot
 * with the particle filter on the same input (added symbols: no struct and no existing signature changed, the ABI number stays).
 * PRECONDITION: that of slam2d_score_poses (a FULL build -- slam2d_field_build or slam2d_field_build_distance -- has run for slot
 * p_field of `level`, ordered in front of the call); the same members of `level` are read.  No Slam2dLidar is taken.  Integer
 * operations and ONE rounded IEEE operation at a time, as in the scan forms: the same inputs give the same bits on every call.
 * slam2d_score_points is slam2d_score_poses with that endpoint: for pose n = (x, y, th) at d_pose[n * pose_stride + 0..2] and its
 * set at d_points + n * set_stride (set_stride 0: the one set for every pose; >= M * point_stride doubles: a set per pose), steps
 * 1-3 of the point cost give valid, the INSIDE points, their cells and sum_b; U = the SET of cells of the inside points, sum_u its
 * sum; d_out[n * SLAM2D_SCORE_STRIDE + 0..7] as slam2d_score_poses lists them, with the number of VALID points in slot 4.  ONE
 * launch, a wave per pose with a hash set of score_hash_size(M) keys of its own, no global atomic; a pose costs one cos / sin.
 * slam2d_mcl_step_points is slam2d_mcl_step with steps a (NOISE), b (MOVE), d (RESAMPLE) and e (REPORT) as written there and
 *   c. WEIGH.  For the moved pose (x', y', th') and the ONE set d_points, steps 1-4 of the point cost, with c = cos(th'), s =
 *      sin(th'):  cost_n = sum_b + (uint64)(valid - inside) * outside_cost;  cmin, best and w_n as in slam2d_mcl_step.
 *   Report word 5 is `valid`.  A set without a valid point costs 0 at every pose: every weight is d_lut[0], best = 0, and the
 *   resampling is the one of equal weights.
 * d_work: slam2d_mcl_points_work(N) = slam2d_mcl_work(N) + 2 * N 8-byte words: behind the scan form's arrays the move launch
 * leaves cos(th'), sin(th') of every MOVED heading, so the scoring launch -- a wave per particle, the points interleaved over
 * its lanes -- reads four doubles per particle and evaluates no transcendental (a set's trip of 64 points is cheaper than the
 * pair); the sixteen waves of a block join their packed minima in LDS in front of the block's one integer atomicMin.  Five
 * launches, of which the weigh and resample launches are slam2d_mcl_step's own kernels.
 * slam2d_mcl_step_adaptive_points is slam2d_mcl_step_adaptive with the same WEIGH step and word 5; its EQUIVALENCE clause holds
 * against slam2d_mcl_step_points.  d_work: slam2d_mcl_adapt_points_work(n_cap, bins) = slam2d_mcl_adapt_work(n_cap, bins) +
 * 2 * n_cap words.  Seven launches; the weigh, reference, count and resample launches are slam2d_mcl_step_adaptive's own.
 * All three allocate nothing, raise no fault bit and do not synchronise; the caller need not initialise d_out, d_work, d_report,
 * d_pose_out or d_ancestor.  SLAM2D_E_BADARG, before any HIP call: the level cases of slam2d_score_poses; M < 1 or >
 * SLAM2D_MAX_POINTS, point_stride < 2, a NULL d_points; (score) a NULL d_pose or d_out, N <= 0, pose_stride < 3, set_stride
 * neither 0 nor >= M * point_stride; (steps) every particle, table and motion case of slam2d_mcl_step and, for the adaptive one,
 * every count, table and bins case of slam2d_mcl_step_adaptive.  SLAM2D_E_TOOLARGE: as in the scan forms (the poses of one
 * launch, N or n_cap > SLAM2D_MCL_MAX_PARTICLES, the bins, fmax * fpitch >= 2^29).  The two *_work functions make no HIP call;
 * < 0 means SLAM2D_E_*, as slam2d_mcl_work and slam2d_mcl_adapt_work answer. */
int slam2d_score_points(const Slam2dLevel* level, int32_t p_field, int32_t N,
                        const double* d_pose, int32_t pose_stride,
                        const double* d_points, int32_t point_stride, int32_t M, int32_t set_stride,
                        double* d_out, void* stream);
int64_t slam2d_mcl_points_work(int32_t N);                      /* slam2d_mcl_work(N) + 2 * N */
int slam2d_mcl_step_points(const Slam2dLevel* level, int32_t p_field, int32_t N,
                           const double* d_pose_in, double* d_pose_out, int32_t pose_stride,
                           const double motion[3], const double amp[3], uint64_t seed, uint64_t scan,
                           const double* d_points, int32_t point_stride, int32_t M,
                           uint32_t outside_cost, const uint32_t* d_lut, int32_t lut_n, int32_t lut_shift,
                           int32_t* d_ancestor, uint64_t* d_work, uint64_t* d_report, void* stream);
int64_t slam2d_mcl_adapt_points_work(int32_t n_cap, const Slam2dMclBins* bins);   /* slam2d_mcl_adapt_work(n_cap, bins) + 2 * n_cap */
int slam2d_mcl_step_adaptive_points(const Slam2dLevel* level, int32_t p_field, int32_t n_cap,
                                    const uint32_t* d_n_in, uint32_t* d_n_out,
                                    const double* d_pose_in, double* d_pose_out, int32_t pose_stride,
                                    const double motion[3], const double amp[3], uint64_t seed, uint64_t scan,
                                    const double* d_points, int32_t point_stride, int32_t M,
                                    uint32_t outside_cost, const uint32_t* d_lut, int32_t lut_n, int32_t lut_shift,
                                    const Slam2dMclBins* bins, const uint32_t* d_ntab, int32_t ntab_n,
                                    int32_t* d_ancestor, uint64_t* d_work, uint64_t* d_report, void* stream);

/* Exact wall distances as a search field: another way to fill the slots of a level, for the calls that read a full field
 * (slam2d_score_poses, slam2d_search_lattice, slam2d_mcl_step, slam2d_mcl_step_adaptive) -- the likelihood field of Monte-Carlo
 * localisation (Thrun, Burgard, Fox, Probabilistic Robotics, 6.4) instead of the blurred probSP, whose reach ends at
 * SLAM2D_MAX_BLUR_RADIUS cells; and, through d_dist2, the clearance map of the occupancy grid.  An added symbol: no struct and no
 * existing signature changed, the ABI number stays.  For particle p:
 *   a. frame, axis tables and occupied image are what slam2d_field_build produces for the same arguments: level->frames[p] as the
 *      frame kernel leaves it (field_min = floor_value, redo = 0, min_known = 0, field_max = 0: zero bounds every field value from
 *      above; the call does not measure the field), axis_x, axis_y, and a byte of level->occ[p] equals the generation stamp
 *      (occ_gen, or 1 when occ_gen == 0) iff a map cell of the window is occupied there (occ_bits); the memset when occ_gen == 0
 *      and the 8 x 8 block flags (tilemask) as in the full build; the same fault bits in d_flags[p]
 *      (SLAM2D_F_WINDOW_OUTSIDE_MAP, SLAM2D_F_FIELD_INDEX);
 *   b. with O the set of occupied field cells (a, b) in [0, fh) x [0, fw): d2(i, j) = min over O of (a - i)^2 + (b - j)^2, an
 *      exact integer (below 2^31 within fmax * fpitch < 2^29), +inf when O is empty; k(i, j) = min(d2(i, j), lut_n - 1);
 *   c. field[p][i * fpitch + j] = d_lut[k(i, j)] for every (i, j) in [0, fh) x [0, fw) and, where d_dist2 is not NULL,
 *      d_dist2[(p * fmax + i) * fpitch + j] = k(i, j).  Cells of either image outside the frame are unspecified; nothing outside
 *      the P * fmax * fpitch words of either image is written;
 *   d. the slots are handed back as SearchLevel.set_field does on the host: their tilestate is set to 1 and, where freerow is not
 *      NULL, their freerow rows are zeroed, so a later slam2d_field_build or slam2d_match on the level rebuilds the reference's
 *      field from scratch and finds no tile that supposedly holds the free-space constant.
 * PRECONDITION of the consumers: the field holds costs at level->cost_scale -- the caller puts its table's scale there before it
 * calls them (the build itself does not read cost_scale beyond slam2d_field_build's own check).
 * Every join is a minimum of integers: the same inputs give the same bits on every call.  The result is clamped at lut_n - 1 <=
 * 65535, so no cell needs occupancy farther than R = ceil(sqrt(lut_n - 1)) <= 256 rows or columns away: a column pass (rows to
 * the nearest occupied cell of the column, saturated at R + 1, kept in `field`) and a row pass (min over |b - j| <= R of
 * (b - j)^2 + g(i, b)^2, a row per block in LDS), each a launch of its own behind the frame and scatter launches.  No floating
 * point.  Allocates nothing, does not synchronise, raises no fault bit beyond a.  SLAM2D_E_BADARG, before any HIP call: every
 * case slam2d_field_build refuses, by the same checks, a NULL d_lut, lut_n < 1 or > SLAM2D_DISTANCE_MAX_TABLE, a level without
 * frames, axis_x, axis_y or field, occ_gen outside 0 .. 255;
 * SLAM2D_E_TOOLARGE: as in slam2d_field_build. */
#define SLAM2D_DISTANCE_MAX_TABLE 65536
int slam2d_field_build_distance(const Slam2dLidar* lidar, const Slam2dLevel* level, const Slam2dMap* d_maps, int32_t P,
                                const double* d_centre, int32_t centre_stride,
                                const uint32_t* d_lut, int32_t lut_n, uint32_t* d_dist2,
                                uint32_t* d_flags, void* stream);

/* Particle.updateEstimatedPose for P particles (Algorithm/FastSlam.py:77-106): the pose prior of the
 * next scan from the previous matched poses and the raw odometry increment.
 *   d_prev_pose[p*3 + 0..2]  previous matched pose (prevMatchedReading)
 *   raw_theta, prev_raw_theta  currentRawReading['theta'], prevRawReading['theta'] (:78)
 *   has_turn / raw_turn      rawMovingTheta - prevRawMovingTheta when both exist (:94), else has_turn = 0
 *   d_heading[P]             prevMatchedMovingTheta per particle, NaN for None
 * Writes d_est[p*3 + 0..2] (estimatedReading pose) and d_psi_cs[p*2 + 0..1] = (cos, sin) of
 * estMovingTheta (NaN pair for None), the inputs of slam2d_field_build / slam2d_sweep. */
int slam2d_prior(const double* d_prev_pose, double raw_theta, double prev_raw_theta, int32_t has_turn,
                 double raw_turn, const double* d_heading, int32_t P, double* d_est, double* d_psi_cs,
                 void* stream);

/* The bookkeeping after a match (Algorithm/FastSlam.py:108-120,131-135): heading of the matched step
 * (getMovingTheta), previous pose <- matched pose, log-weight += log coarse confidence.
 *   d_fine / d_coarse        Slam2dMatch[P] of the fine / coarse level
 *   d_prev_pose[P][3]        in: previous matched pose, out: this scan's matched pose
 *   d_heading[P]             out: prevMatchedMovingTheta (NaN when the pose did not move)
 *   d_logw[P]                in/out
 *   d_report[P][5]           out (may be NULL): matched x, y, theta, coarse confidence, log of it -- the one
 *                            buffer a caller needs to download per scan */
int slam2d_post_match(const Slam2dMatch* d_fine, const Slam2dMatch* d_coarse, int32_t P, double* d_prev_pose,
                      double* d_heading, double* d_logw, double* d_report, void* stream);

/* Particle.update's `weight *= confidence` in the log domain followed by
 * ParticleFilter.normalizeWeights / weightUnbalanced (Algorithm/FastSlam.py:30-48,135).
 *   d_logw[N]    in/out: log-weights of ALL N particles (after an all-gather when sharded)
 *   d_logconf    log-confidences to add first, element i at d_logconf[i*logconf_stride] (NULL: none)
 *   d_w[N]       out: normalised weights
 *   d_stats[2]   out: [variance = sum (w - 1/N)^2, log of the pre-normalisation weight sum] */
int slam2d_weights_normalize(double* d_logw, const double* d_logconf, int32_t logconf_stride, int32_t N,
                             double* d_w, double* d_stats, void* stream);
/* slam2d_grid_update and slam2d_weights_normalize in ONE launch (the normaliser is one extra block beside the
 * update's: it only reads the log-weights and the log-confidences, which the match wrote).  N = P. */
int slam2d_grid_update_weights(const Slam2dLidar* lidar, const Slam2dMap* d_maps, int32_t P, const double* d_pose,
                               int32_t pose_stride, const double* d_ranges, uint32_t* d_flags, double* d_logw,
                               const double* d_logconf, int32_t logconf_stride, double* d_w, double* d_stats, void* stream);
/* The same for particles sharded over processes: the extra block is slam2d_weights_local (d_part[3] out); the caller's
 * all-gather and slam2d_weights_merge follow. */
int slam2d_grid_update_weights_local(const Slam2dLidar* lidar, const Slam2dMap* d_maps, int32_t P, const double* d_pose,
                                     int32_t pose_stride, const double* d_ranges, uint32_t* d_flags, double* d_logw,
                                     const double* d_logconf, int32_t logconf_stride, double* d_part, void* stream);

/* One scan of Particle.update for P particles in two calls (Algorithm/FastSlam.py:122-135), so that a host loop pays two
 * library calls per scan instead of six:
 *   slam2d_scan_match   = slam2d_prior + slam2d_match(coarse; soft-max draw if d_uniform) + slam2d_match(fine, centred on
 *                         the coarse result, arg-max) -- reads the maps, changes no filter state; `options` as slam2d_match
 *                         (coarse level);
 *   slam2d_scan_commit  = slam2d_post_match + slam2d_grid_update at the matched poses + (d_w != NULL) slam2d_weights_normalize
 *                         over these P particles (in the update's launch), which also moves the scan's fault bits from
 *                         d_flags into d_flag_snapshot[P] with an atomic exchange, so that one asynchronous download
 *                         returns everything the host reads; a bit the update raises after the exchange stays in d_flags
 *                         and is reported with the next call.
 *                         abort_mask (d_w != NULL only; 0: none): SLAM2D_F_* bits that void the scan.  A driver that enqueues
 *                         the commit before it has seen the match's fault bits (the pipelined closed loop) passes
 *                         SLAM2D_F_WINDOW_OUTSIDE_MAP: if the match raised such a bit for ANY particle -- the reference would
 *                         have grown that map first (checkAndExapndOG, Utils/ScanMatcher_OGBased.py:27) -- the whole launch is
 *                         a no-op (no bookkeeping, no map update, no weights; d_flag_snapshot receives the bits, d_flags keeps
 *                         them) and the host grows the maps and runs the scan again.  ABI 13: the voided launch leaves the
 *                         COARSE matched poses in d_report[i][0..2] (the other columns keep their old content): what the host
 *                         needs to grow the maps for the fine windows (:27 at the fine level) without matching again.
 * Arguments as in the calls they bundle. */
int slam2d_scan_match(const Slam2dLidar* lidar, const Slam2dLevel* coarse, const Slam2dLevel* fine, const Slam2dMap* d_maps,
                      int32_t P, const double* d_prev_pose, double raw_theta, double prev_raw_theta, int32_t has_turn,
                      double raw_turn, const double* d_heading, const double* d_ranges, double est_moving_dist,
                      const double* d_uniform, double* d_est, double* d_psi_cs, Slam2dMatch* d_coarse, Slam2dMatch* d_fine,
                      uint32_t* d_flags, uint32_t options, void* stream);
int slam2d_scan_commit(const Slam2dLidar* lidar, const Slam2dMap* d_maps, int32_t P, const Slam2dMatch* d_fine,
                       const Slam2dMatch* d_coarse, double* d_prev_pose, double* d_heading, double* d_logw, double* d_report,
                       const double* d_ranges, uint32_t* d_flags, double* d_w, double* d_stats, uint32_t* d_flag_snapshot,
                       uint32_t abort_mask, void* stream);

/* slam2d_scan_commit that ALSO writes the next scan's pose prior (slam2d_prior's work: Algorithm/FastSlam.py:77-106 needs only
 * this scan's matched poses and headings and the next reading's odometry, which a driver replaying a log -- or one scan behind a
 * live sensor -- holds when it commits): the bookkeeping block computes d_next_est[P][3] / d_next_psi_cs[P][2] behind each
 * particle's bookkeeping, and the next slam2d_scan_match is called with SLAM2D_MATCH_PRIOR_READY -- one launch less per scan.
 * A voided scan (abort_mask) writes no prior; the driver re-issues it without the option.  d_next_est NULL: slam2d_scan_commit. */
int slam2d_scan_commit_next(const Slam2dLidar* lidar, const Slam2dMap* d_maps, int32_t P, const Slam2dMatch* d_fine,
                            const Slam2dMatch* d_coarse, double* d_prev_pose, double* d_heading, double* d_logw, double* d_report,
                            const double* d_ranges, uint32_t* d_flags, double* d_w, double* d_stats, uint32_t* d_flag_snapshot,
                            uint32_t abort_mask, double next_raw_theta, double next_prev_raw_theta, int32_t next_has_turn,
                            double next_raw_turn, double* d_next_est, double* d_next_psi_cs, void* stream);

/* The same normaliser for particles sharded over several processes (one per GPU).  Rank-local
 * half: d_logw[i] += d_logconf[i * logconf_stride], then d_part[3] = [max log w, sum exp(lw - max),
 * sum exp(2 (lw - max))] of this rank's N particles.  The caller all-gathers the 24 bytes of every
 * rank (the only collective of a scan) and hands the [world][3] array to slam2d_weights_merge,
 * which folds it in rank order, writes this rank's normalised weights / log-weights and
 * d_stats[2] = [sum over ALL particles of (w - 1/total)^2, log of the pre-normalisation sum].
 * slam2d_weights_local: a log-weight of -inf counts as weight 0 -- a rank of nothing but -inf leaves [-inf, 0, 0] -- a NaN makes the rank's sums NaN.
 * slam2d_weights_merge: -inf particles get weight 0 and log-weight -inf if any particle of any rank is finite; one NaN, or -inf everywhere, makes every rank's weights and d_stats NaN. */
int slam2d_weights_local(double* d_logw, const double* d_logconf, int32_t logconf_stride, int32_t N,
                         double* d_part, void* stream);
int slam2d_weights_merge(double* d_logw, int32_t N, const double* d_parts, int32_t world,
                         int64_t total_particles, double* d_w, double* d_stats, void* stream);
/* The sharded normaliser of particle GROUPS without events between the groups' streams and the normaliser's (round 5; see
 * Slam2dScan.d_norm_sync with merge == 0): slam2d_norm_gate enqueues a one-wave kernel that waits until the normaliser blocks of all
 * G groups of the scan issued just before have left their partials (they count themselves in d_norm_sync[0]); the caller's
 * all-gather of the partials follows on that stream, then slam2d_weights_merge_publish = slam2d_weights_merge + the word the groups'
 * next normaliser blocks wait for (d_norm_sync[1]).  Call both, in this order, once per scan, behind slam2d_groups_step / _commit. */
int slam2d_norm_gate(uint32_t* d_norm_sync, int32_t G, void* stream);
int slam2d_weights_merge_publish(double* d_logw, int32_t N, const double* d_parts, int32_t world, int64_t total_particles,
                                 double* d_w, double* d_stats, uint32_t* d_norm_sync, void* stream);
/* ... and the closed loop's report (ABI 17): slam2d_weights_merge_publish, after which the same block copies d_pack[0 .. pack_doubles)
 * to the pinned host buffer h_pack and stores report_seq into the pinned host word h_seq (system scope) -- what the merging
 * normaliser block does on one rank (Slam2dScan.h_seq).  A sharded rank's commit is slam2d_groups_commit (merge == 0, h_seq NULL),
 * slam2d_norm_gate, the all-gather of the partials, this call; the host waits with slam2d_host_wait_seq.  The NEXT commit may be
 * issued only after that wait has returned: its groups rewrite d_pack's report rows and fault-bit snapshot.
 * A scan VOIDED on some rank (abort_mask: a search window had left a map): that rank's groups leave the void partial (sum -1)
 * and still arrive, so the enqueued gate, collective and merge run on every rank; the merge then changes no weight, publishes
 * nothing to the groups and reports d_stats = [NaN, -1].  The voiding rank grows its maps and issues the scan again (match, commit,
 * gate, all-gather, this call); every OTHER rank -- its own commit stands, its partials are intact, its groups' next normaliser
 * blocks wait -- answers a voided report with the all-gather and this call alone (no gate).  One all-gather per attempt and rank. */
int slam2d_weights_merge_publish_report(double* d_logw, int32_t N, const double* d_parts, int32_t world, int64_t total_particles,
                                        double* d_w, double* d_stats, uint32_t* d_norm_sync, const double* d_pack, double* h_pack,
                                        int32_t pack_doubles, uint32_t* h_seq, uint32_t report_seq, void* stream);

/* ---- one scan for several particle GROUPS, each on its own HIP stream, issued from C in ONE call ----
 * Particles are independent during a scan (Algorithm/FastSlam.py:25-27); every kernel of the step is latency- or issue-bound
 * at a few dozen particles, so a host driver steps its particles in G groups on G streams and joins them only in the weight
 * normaliser (:30-48).  Issued call by call from Python that costs ~7 us of interpreter + ctypes time per launch (round 3:
 * 0.103 of a 0.131 ms step); these entry points issue the same launches for all groups from C, so the host pays one call per
 * scan (slam2d_groups_step) or two (match / commit: the pipelined closed loop reads the previous scan's report in between).
 *
 * A group is described by HOST pointers to its level descriptors -- either levels of its own or offset views of a larger
 * level (every per-particle pointer advanced by the group's first particle; `tilemask` then no longer follows `occ`
 * contiguously, which is accepted whenever occ_gen != 0: nothing is cleared) -- and by device pointers to its slices of the
 * per-particle arrays. */
typedef struct {
    const Slam2dLevel* coarse;   /* HOST pointer */
    const Slam2dLevel* fine;     /* HOST pointer; NULL: single-level match (the coarse result is the matched pose) */
    const Slam2dMap*   d_maps;   /* the group's P map descriptors */
    int32_t P;
    int32_t est_stride;          /* doubles per row of d_est (>= 3) */
    const double* d_est;         /* [P][est_stride] pose estimates handed in (open loop), or NULL: derive them from d_prev_pose
                                    (slam2d_prior) into d_est_out / d_psi_out -- the closed loop */
    const double* d_psi_cs;      /* [P][2] heading prior with d_est (NULL: None); ignored in the closed loop */
    const double* d_uniform;     /* [P] soft-max draw at the coarse level; NULL: arg-max */
    double* d_prev_pose;         /* closed loop: [P][3] previous matched poses, in/out (slam2d_post_match) */
    double* d_heading;           /* closed loop: [P] prevMatchedMovingTheta, in/out */
    double* d_est_out;           /* closed loop: [P][3] */
    double* d_psi_out;           /* closed loop: [P][2] */
    Slam2dMatch* d_coarse;       /* [P] */
    Slam2dMatch* d_fine;         /* [P]; unused when fine == NULL */
    uint32_t* d_flags;           /* [P] fault bits of this scan (the caller alternates two buffers between scans when groups may
                                    run a scan apart and abort_mask is used: see Slam2dScan.d_abort_flags) */
    double* d_logw;              /* [P] log-weights, a slice of Slam2dScan.d_logw_all */
    double* d_part;              /* [3] out: this group's [max log w, sum, sum of squares] (slam2d_weights_local) */
    double* d_report;            /* closed loop: [P][5] (slam2d_post_match) or NULL */
    uint32_t* d_flag_snapshot;   /* closed loop: [P] the scan's fault bits, moved out of d_flags by the commit, or NULL */
    void* stream;                /* the group's HIP stream */
    void* ev_matched;            /* slam2d_event_create(): recorded behind the group's match (needed with abort_mask) or NULL */
    void* ev_done;               /* recorded behind the group's map update */
    /* ABI 16, with Slam2dScan.h_ranges (closed loop only): */
    double* d_pull;              /* [beams] the group's own device copy of the scan's ranges, written by its prior launch (or by the
                                    previous commit, d_pull_next) and read by every later kernel of the group's scan (d_uniform and
                                    Slam2dScan.d_ranges are then ignored) */
    const double* h_uniform;     /* PINNED HOST [P]: the group's soft-max uniforms of this scan (read there by the selecting kernel,
                                    once per particle), or NULL: arg-max */
    double* d_pull_next;         /* [beams] with Slam2dScan.h_next_ranges: where the commit leaves the NEXT scan's ranges -- that
                                    scan's d_pull (the caller alternates two buffers) */
} Slam2dGroup;

/* What all groups of a scan share. */
typedef struct {
    const double* d_ranges;      /* [beams] */
    double est_moving_dist;
    double raw_theta, prev_raw_theta, raw_turn;   /* closed loop: arguments of slam2d_prior */
    int32_t has_turn;
    uint32_t options;            /* as slam2d_match (coarse level) */
    uint32_t abort_mask;         /* closed loop: as slam2d_scan_commit, decided over d_abort_flags[0 .. n_abort_flags): the fault
                                    bits of ALL groups (their d_flags are slices of that array).  Every group's commit waits for
                                    every group's ev_matched first */
    int32_t n_abort_flags;
    const uint32_t* d_abort_flags;
    void* ev_inputs;             /* NULL, or an event every group's stream waits for before its match (inputs staged elsewhere) */
    /* the weight normaliser over all groups (and, sharded, all ranks): slam2d_weights_merge on norm_stream behind every
     * group's update */
    double* d_logw_all;          /* [n_local] the groups' log-weights, consecutive */
    int32_t n_local;
    int32_t n_parts;             /* partials in d_parts: G x ranks */
    const double* d_parts;       /* [n_parts][3]; one rank: the groups' d_part are its rows */
    int64_t total_particles;
    double* d_w;                 /* [n_local] out */
    double* d_stats;             /* [2] out */
    void* norm_stream;
    void* ev_merged;             /* recorded behind the merge; a group's update waits for the previous scan's */
    int32_t wait_merged;         /* 0: first scan, nothing to wait for */
    int32_t merge;               /* 1: issue the merge here.  0: the caller does (sharded: an all-gather of the partials comes
                                    first); norm_stream is still ordered behind every group's ev_done */
    uint32_t* d_norm_sync;       /* NULL, or 64 device words, ZEROED ONCE, kept for the life of these groups (ABI 15): with merge == 1 and
                                    no abort_mask (ABI 16: or abort_mask with match_seq) the groups' normaliser blocks merge among themselves on the device -- the block
                                    that arrives last merges for all -- and a group's next update waits for that inside its own
                                    normaliser block: no merge launch, no norm_stream, no ev_merged / ev_done / wait_merged (they may
                                    be NULL / 0; ev_done is still recorded when given).  d_w / d_stats / the log-weights are final
                                    once EVERY group's stream has passed the scan.  Needs n_parts == G, the groups' d_part being
                                    rows 0 .. G-1 of d_parts.  With merge == 0 (sharded) the groups only wait and arrive through
                                    the words; the caller follows with slam2d_norm_gate, its collective, slam2d_weights_merge_publish.
                                    Use it for every scan of the groups or for none.  At most 56 groups.  The device-side waits are
                                    bounded: word 59 holds the bound in milliseconds (the caller may set it once, before the first
                                    scan; 0 = 30 s); after it a group's fault word 0 receives SLAM2D_F_SYNC_TIMEOUT (word 62 carries
                                    it from the gate) and, where an abort_mask is in use, the scan is voided so that its report
                                    still reaches the host */
    /* ---- ABI 16: the closed loop without events and without copies (all optional; 0 / NULL = as before) ----
     * Measured in round 5: an event packet between two kernels of a stream costs 3 us, a wait across streams 6-8 us, a copy-engine
     * transfer in front of a kernel ~10 us; a grouped closed-loop scan had ten of them. */
    const double* h_ranges;      /* PINNED HOST [beams], device-visible (hipHostMalloc / torch pin_memory): every group's prior launch
                                    pulls the ranges and Slam2dGroup.h_uniform into Slam2dGroup.d_pull -- no staging copy, no ev_inputs.
                                    The caller alternates two host buffers between scans (a group may still be pulling scan s
                                    while the host stages s + 1) */
    uint32_t match_seq;          /* != 0 (needs d_norm_sync): the number of slam2d_groups_match[_begin] calls with match_seq != 0 since
                                    d_norm_sync was zeroed, this one included, passed AGAIN to the commit of the same scan.  In the
                                    match, the wave that writes a particle's result at the last level counts the particle in (word
                                    61); every group's commit starts with a one-wave gate kernel that waits (bounded) for
                                    n_abort_flags * match_seq arrivals: the abort_mask decision over all groups' fault bits without
                                    ev_matched, and d_norm_sync's device-side merge stays usable with abort_mask (a voided scan has no
                                    normaliser: nobody arrives there, the words stay in step).  n_abort_flags = all groups' particles */
    uint32_t report_seq;         /* with h_seq: the value to publish for this scan (the caller counts its commits) */
    uint32_t* h_seq;             /* PINNED HOST word, or NULL.  (The caller waits for scan s's value before it issues the commit of scan
                                    s + 1: that commit's groups rewrite the report rows and the fault-bit snapshot inside d_pack.)
                                    With d_norm_sync and merge == 1: the block that finishes the scan for
                                    all groups (the merging normaliser block; for a voided scan the last group's block 0, counted in
                                    word 60) copies d_pack[0 .. pack_doubles) to h_pack and then stores report_seq here, system scope.
                                    The host waits with slam2d_host_wait_seq: no download, no event */
    double* h_pack;              /* PINNED HOST [pack_doubles] */
    const double* d_pack;        /* device [pack_doubles]: whatever the caller wants of the scan -- it lays d_report, d_w, d_stats and
                                    d_flag_snapshot out inside this buffer */
    int32_t pack_doubles;
    /* commit only, closed loop with h_ranges: the NEXT scan's prior (slam2d_prior's arguments for it) and ranges ride in this
     * commit's bookkeeping block -- into every group's d_est_out / d_psi_out and d_pull_next -- and the next match is called with
     * SLAM2D_MATCH_PRIOR_READY in `options`: one launch less per group and scan.  A voided scan writes neither: the caller
     * re-issues without the option.  NULL: no such thing */
    const double* h_next_ranges; /* PINNED HOST [beams] */
    double next_raw_theta, next_prev_raw_theta, next_raw_turn;
    int32_t next_has_turn;
} Slam2dScan;

/* match of every group (prior when d_est == NULL, coarse level, fine level) on its stream; records ev_matched */
int slam2d_groups_match(const Slam2dLidar* lidar, const Slam2dGroup* groups, int32_t G, const Slam2dScan* scan);
/* map update at the matched poses + bookkeeping + the group's normaliser partial in ONE launch per group (closed loop:
 * slam2d_scan_commit's work with the abort decided over all groups), then the merge.  */
int slam2d_groups_commit(const Slam2dLidar* lidar, const Slam2dGroup* groups, int32_t G, const Slam2dScan* scan);
/* slam2d_groups_match, but the call returns while worker threads still issue the launches (all groups on workers; the
 * descriptors are copied, the level descriptors they point to must stay untouched until the join).  The next slam2d_groups_* call
 * waits for them first and returns their error; slam2d_groups_join does only that -- call it before synchronising the device or
 * touching anything the match reads.  Without worker threads (slam2d_group_policy) the call is slam2d_groups_match. */
int slam2d_groups_match_begin(const Slam2dLidar* lidar, const Slam2dGroup* groups, int32_t G, const Slam2dScan* scan);
int slam2d_groups_join(void);
/* Host side of Slam2dScan.h_seq: spin until the word has reached `want` (wrap-safe); SLAM2D_E_TIMEOUT after timeout_s seconds. */
int slam2d_host_wait_seq(const uint32_t* h_seq, uint32_t want, double timeout_s);
/* both, group by group (a group's update is enqueued right behind its match): the open-loop step of bench.py */
int slam2d_groups_step(const Slam2dLidar* lidar, const Slam2dGroup* groups, int32_t G, const Slam2dScan* scan);
/* How these three calls issue their groups on this host (decided at the first call; one call runs at a time, a second caller
 * waits).  out4[0] = host cores this process may use (scheduler affinity capped by the cgroup CPU quota), out4[1] = processes
 * assumed to share them (SLAM2D_LOCAL_RANKS, else torchrun's LOCAL_WORLD_SIZE, else 1), out4[2] = 1: one worker thread per group
 * beyond the first issues that group's launches (needs >= 3 cores per process: a worker and the waiting caller both poll;
 * otherwise all groups are issued from the calling thread), out4[3] = 1: the threads poll briefly and yield (< 6 cores per
 * process).  SLAM2D_GROUP_THREADS=0 / 1 forces out4[2]. */
int slam2d_group_policy(int32_t* out4);

/* ParticleFilter.resample's state movement (Algorithm/FastSlam.py:56-61) for maps of
 * identical shape: dst[p] = src[d_index[p]].  Ragged maps are copied by the host with
 * plain device-to-device copies instead. */
int slam2d_gather_maps(const Slam2dMap* d_src, const Slam2dMap* d_dst, const int32_t* d_index,
                       int32_t P, int64_t cells_per_map, void* stream);

/* Recompute occ_bits from cells for the maps d_maps[d_index[0..n)] (d_index NULL: maps 0..n-1).
 * Needed after the caller wrote `cells` itself (upload, growth copy, resample copy). */
int slam2d_map_refresh_bits(const Slam2dMap* d_maps, const int32_t* d_index, int32_t n, void* stream);

/* The picture of particle p's map that the reference's driver draws per scan (Algorithm/FastSlam.py:172-177:
 * `ogMap = visited / total; ogMap = ogMap[y0:y1, x0:x1]; np.flipud(1 - ogMap)`), straight from the device state:
 *   d_out[i][j]    (float64, may be NULL) = 1 - visited / total of map cell (row, x0 + j), row = y0 + i, or -- flipud != 0 --
 *                  y1 - 1 - i; the window [y0, y1) x [x0, x1) must lie inside the map (the caller resolves Python's slice
 *                  clipping, as convertRealXYToMapIdx + slicing do there);
 *   d_out_u8[i][j] (may be NULL) the same as 8-bit grey, rint(255 * value). */
int slam2d_map_image(const Slam2dMap* d_maps, int32_t p, int32_t x0, int32_t x1, int32_t y0, int32_t y1, int32_t flipud,
                     double* d_out, uint8_t* d_out_u8, void* stream);

/* ABI 13: expandOccupancyGrid (Utils/OccupancyGrid.py:59-100) for the count array, a whole growth SEQUENCE at once: every cell
 * of the caller-allocated new map (descriptors in HOST memory; new_map->cells [rows][pitch], new_map->occ_bits [rows][bits_pitch])
 * is written in one pass -- the old map's cell (r, c) at (r + d_row, c + d_col) (d_row / d_col: rows / columns the sequence
 * inserted on the low sides, :70-71; the high sides are appended, :81-82), SLAM2D_INIT_CELL elsewhere, pitch padding included --
 * together with the new map's occupancy bits.  Both maps in the same cell format (`wide`). */
int slam2d_map_grow(const Slam2dMap* old_map, const Slam2dMap* new_map, int32_t d_row, int32_t d_col, void* stream);

/* Fill a map with SLAM2D_INIT_CELL (np.ones / 2*np.ones, Utils/OccupancyGrid.py:13-14). */
int slam2d_map_fill(uint32_t* d_cells, int64_t n, uint32_t value, void* stream);

/* cos / sin of n angles as the endpoint kernel evaluates them on the device (ocml, fp64).  Test aid: the
 * reference evaluates them with NumPy (Utils/ScanMatcher_OGBased.py:87-88); tests measure the distance. */
int slam2d_device_sincos(const double* d_angles, int32_t n, double* d_cos, double* d_sin, void* stream);

/* Per-stage timing for bench.py's roofline figure: when a stage's bit is enabled, every
 * launch of that stage's kernel is bracketed by a HIP event pair on the launch stream
 * (up to `capacity` launches).  slam2d_prof_collect synchronises on the recorded
 * events, returns their summed duration and launch count, and resets the stage. */
#define SLAM2D_STAGE_SWEEP     0   /* k_sweep: pose-cube scoring */
#define SLAM2D_STAGE_BLUR      1   /* k_blur_clamp: separable blur + clamp */
#define SLAM2D_STAGE_SCATTER   2   /* k_occ_scatter: map window -> occupied field cells */
#define SLAM2D_STAGE_UPDATE    3   /* k_grid_update: occupancy-grid update */
#define SLAM2D_STAGE_SELECT    4   /* k_select: argmax / soft-max draw / confidence */
#define SLAM2D_STAGE_ENDPOINTS 5   /* k_endpoints: unique endpoint cells */
#define SLAM2D_STAGE_BOUND     6   /* k_bound: tile upper bounds + seed tiles (branch and bound) */
#define SLAM2D_STAGE_EXACT     7   /* k_exact: exact scores of the surviving tiles + selection */
#define SLAM2D_STAGE_COUNT     8
int  slam2d_prof_enable(uint32_t stage_mask, int32_t capacity);
int  slam2d_prof_collect(int32_t stage, double* total_ms, int32_t* launches);
/* Sample: only every `every`-th launch of an enabled stage gets its event pair (default 1).  An event pair costs the
 * stream ~6 us on each side of the kernel; a timed region that must not carry that on every step samples instead. */
int  slam2d_prof_every(int32_t every);
void slam2d_prof_disable(void);

/* Ordering between streams for a host driver that runs groups of particles on several HIP streams (particles are
 * independent during a scan, Algorithm/FastSlam.py:25-27; only the weight normaliser, :30-48, joins them): events without
 * timing.  slam2d_event_record marks a point of `stream`; slam2d_stream_wait_event makes later work of `stream` wait for it. */
/* n non-blocking streams for particle groups, PLACED on the runtime's hardware queues by measurement (round 8; before: created in one
 * batch and hoped to land on distinct queues -- at the runtime's default of four queues two groups of four shared one and took turns).
 * A bounded overlap probe (a ~150 us spin kernel on one stream, a time stamp on the other: the stamp precedes the spin's end only on
 * another queue) sorts the streams into queue classes; where the batch holds fewer than four classes, further streams and then
 * streams at the greatest priority are created, probed, and destroyed again if not handed out.  out[1..4] sit on pairwise distinct
 * queues (the group streams of a two- and of a four-group run); out[0] (the normaliser's) not on the queue of out[1] or out[2]; the
 * rest in any order.  Where four queues cannot be had (GPU_MAX_HW_QUEUES below 4) the best placement found is returned: no error.
 * More than four groups still take turns at four queues: an application that can should set GPU_MAX_HW_QUEUES=8 before its first
 * HIP call.  Costs about 10 ms (the first batch of a process 20-160 ms); a host driver calls it ONCE per process and device and reuses the streams.
 * slam2d_streams_queue_classes: for n streams, the queue class of each in the LAST batch (-1: not of it) and the number of classes
 * that batch found; stats is NULL or 6 words: tier that supplied the last class (0 the plain batch, 1 further streams, 2 priority
 * streams), probes run, candidates created, candidates destroyed, microseconds taken, streams among out[1..4] that share a queue
 * with an earlier one.  It makes no HIP call.  (An added symbol: no struct and no existing signature changed, the ABI number stays.) */
int   slam2d_streams_create(void** out, int32_t n);
int   slam2d_streams_queue_classes(void* const* streams, int32_t n, int32_t* out_class, int32_t* n_classes, int32_t* stats);
void  slam2d_stream_destroy(void* stream);
void* slam2d_event_create(void);
void  slam2d_event_destroy(void* event);
int   slam2d_event_record(void* event, void* stream);
int   slam2d_stream_wait_event(void* stream, void* event);

/* Timing helper for bench.py: HIP events on the caller's stream.
 * slam2d_timer_create -> opaque handle; _start/_stop record events on `stream`;
 * _elapsed_ms synchronises on the stop event and returns milliseconds. */
void* slam2d_timer_create(void);
void  slam2d_timer_destroy(void* timer);
int   slam2d_timer_start(void* timer, void* stream);
int   slam2d_timer_stop(void* timer, void* stream);
int   slam2d_timer_elapsed_ms(void* timer, float* ms);

#ifdef __cplusplus
}
#endif
#endif /* SLAM2D_H */
