// rfec_kernels.hip -- the dispatch of the flex-FEC engine's CDNA4 (gfx950) kernels: the thin extern "C" launch
// shim the C host layer (rfec_host.c) calls picks, by plan, the kernel family a batch takes; each family's
// kernels and launchers live in a unit of their own, whose head says what it does.  Also here: the launch-timing
// state and the dispatch tag.
//  encode (rfec_encode.hip): row layouts, the sender's full rows + columns plan (k = 6..16), any other plan;
//  recover (launch_recover picks by plan):
//    * pairwise disjoint lines (row layer, strip mode), one launch: rfec_fused.hip;
//    * lines that cascade (the sender's rows + columns: k <= 64, <= 8 lines of <= 4 members), one launch:
//      rfec_cascade.hip;
//    * otherwise (and RFEC_TUNE_GENERIC): the peel and the replay of rfec_peel.hip;
//  recover through a slot map over a row pool (rfec_launch_recover_indexed, dense output only): row layouts in
//  one launch (rfec_fused.hip), every other plan the peel and an indexed replay (rfec_peel.hip).  (The sender's
//  matrix plans in one launch are entry points of their own, rfec_launch_recover_indexed_matrix in
//  rfec_cascade.hip for k = 6..16 and rfec_launch_recover_indexed_matrix_wide in rfec_matrix_wide.hip for any
//  k = 6..128: this dispatch does not pick them.)
#include "rfec_families.h"

static thread_local hipEvent_t t_ev_start = nullptr, t_ev_stop = nullptr;
static thread_local uint32_t t_launches = 0; // launches since rfec_timing_events
static thread_local uint32_t t_path = RFEC_PATH_NONE; // the dispatch tag (rfec_internal.h): the last launch's kernel
// rfec_recover_indexed_out's dispatch tag (rfec_internal.h), kept apart from t_path's kinds
static thread_local uint32_t t_indexed_path = 0;

bool rfec_timing_take(hipEvent_t* start, hipEvent_t* stop)
{
    ++t_launches;
    if (!t_ev_start && !t_ev_stop)
        return false;
    *start = t_ev_start;
    *stop = t_ev_stop;
    t_ev_start = t_ev_stop = nullptr;
    return true;
}

void rfec_set_path(uint32_t path) { t_path = path; }
void rfec_set_indexed_path(uint32_t path) { t_indexed_path = path; }

namespace {

// the sender's full plan of a k-segment group in rows of `col`: rows, then
// columns, lines with fewer than 2 members dropped (flex_fec_sender.c:166-233)
bool is_full_matrix(const rfec_kplan* P, uint32_t col)
{
    const uint32_t k = P->k, rows = (k + col - 1) / col;
    uint32_t l = 0;
    for (uint32_t r = 0; r < rows; ++r) {
        const uint32_t cnt = k - r * col < col ? k - r * col : col;
        if (cnt < 2)
            continue;
        if (l >= P->n_lines || P->line[l].first != r * col || P->line[l].stride != 1 || P->line[l].count != cnt)
            return false;
        ++l;
    }
    for (uint32_t c = 0; c < col; ++c) {
        const uint32_t cnt = (k - c + col - 1) / col;
        if (cnt < 2)
            continue;
        if (l >= P->n_lines || P->line[l].first != c || P->line[l].stride != col || P->line[l].count != cnt)
            return false;
        ++l;
    }
    return l == P->n_lines;
}

bool is_row_layout(const rfec_kplan* P, uint32_t* col_out)
{
    const uint32_t col = P->n_lines ? P->line[0].count : 0;
    bool rows = col >= 2 && P->n_lines == (P->k + col - 1) / col;
    for (uint32_t l = 0; l < P->n_lines && rows; ++l) {
        const uint32_t first = l * col;
        const uint32_t count = P->k - first < col ? P->k - first : col;
        rows = P->line[l].stride == 1 && P->line[l].first == first && P->line[l].count == count;
    }
    *col_out = col;
    return rows;
}

hipError_t launch_encode(const EncLaunch& a, unsigned flags)
{
    const rfec_kplan* P = a.P;
    const bool generic = (flags & RFEC_KFLAG_GENERIC) != 0;
    uint32_t col = 0;
    // k_encode_out / k_encode_matrix_out address a wave's groups (at most kWave + 1 of them) through one
    // buffer descriptor of range kNoLoad: per-lane offsets must stay below it, or a large stride would
    // read zeros past the range (the same bound as the fused decodes, launch_recover)
    const bool rsrc_ok = (uint64_t)(kWave + 1) * P->k * a.stride < kNoLoad;
    if (!generic && is_row_layout(P, &col) && col <= 16 &&
        (uint64_t)a.groups * ((P->k + col - 1) / col) * a.cd < (1ull << 32))
        return launch_encode_rows(a, col, rsrc_ok);
    // (the matrix encode's lane count is 32-bit, as the row branch's: a larger batch takes k_encode)
    if (!generic && rsrc_ok && rfec_packed_matrix_col(P) && (uint64_t)a.groups * P->n_lines * a.cd < (1ull << 32))
        return launch_encode_matrix(a);
    return launch_encode_plan(a);
}

int launch_recover(const rfec_kmask* M, uint32_t groups, uint32_t stride, uint32_t capacity, uint8_t* shards,
                   rfec_hdr* hdr, const uint64_t* present, const uint8_t* parity, const rfec_hdr* meta,
                   const uint16_t* fsize, const uint64_t* parity_present, uint64_t* recovered, void* ws,
                   void* stream, unsigned flags, const rfec_dense_out* out)
{
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const bool dense = out && out->per_group;
    const bool generic = (flags & RFEC_KFLAG_GENERIC) != 0;
    const rfec_kplan& P = M->plan;
    PeelArgs B;
    const PeelGeom G = peel_args(&B, *M, groups, capacity, hdr, present, meta, fsize, parity_present, recovered, ws,
                                 out);
    const uint32_t maxc = G.maxc;
    const DenseOut DO = {dense ? reinterpret_cast<v4u*>(out->shards) : nullptr, dense ? out->per_group : 0u};
    const uint32_t C = stride / 16;
    const uint32_t cd = capacity ? (capacity + 15) / 16 : 1;
    // disjoint plans (row layer alone, strip mode), lines of <= 8 members: one launch, header lanes
    // (the fused kernels address a wave's groups through one buffer descriptor: offsets < kNoLoad)
    const bool fused = G.disjoint && maxc <= 8 && !generic &&
                       (uint64_t)(kWave + 1) * (P.k > P.n_lines ? P.k : P.n_lines) * stride < kNoLoad;
    // plans with cascades within the register schedule (the sender's matrix plans): one launch
    const uint32_t Q = dense ? out->per_group : (P.n_lines < P.k ? P.n_lines : P.k);
    const bool cascade = !G.disjoint && maxc <= 4 && P.n_lines <= 8 && P.k <= 64 && !generic &&
                         (uint64_t)groups * Q * cd < (1ull << 32) && (uint64_t)(kWave + 1) * P.k * stride < kNoLoad;
    // everything else (and RFEC_TUNE_GENERIC): the LDS peel + schedule replay, in place or dense
    const v4u* pp = reinterpret_cast<const v4u*>(parity);
    v4u* sh = reinterpret_cast<v4u*>(shards);
    if (fused) { // header lanes, one per (group, line)
        B.nlp_log2 = rfec_header_lanes_log2(P.n_lines);
        const uint32_t n_hdr = blocks_for((uint64_t)groups << B.nlp_log2); // host checks groups << lg < 2^32
        const FusedArgs F = {sh, pp, groups * cd, C, make_fastdiv(cd), n_hdr, st, DO};
        // output-mapped (a lane per (group, line or slot, chunk)) where a line's slot spans at least a wave
        // of chunks; below that most of its lanes would sit on lines that do not fire (k = 32 / 256 B, 2
        // erasures: 6 of 8 rows idle, 60.0 vs 41.6 us flat), so the flat form -- except a dense output of
        // row layouts with slots of >= 16 chunks: lanes per output slot sit on no idle line (k = 32 /
        // 256 B: 33.2-33.9 vs 34.6-34.9 us flat, round 5)
        uint32_t col = 0;
        const bool slots = F.D.E && F.D.E <= P.n_lines; // dense output: lanes per output slot
        const bool rows = !generic && is_row_layout(&P, &col) && col <= 4 && P.k <= 64;
        if ((cd >= (uint32_t)kWave || (slots && rows && cd >= 16)) &&
            (uint64_t)groups * P.n_lines * cd < (1ull << 32)) {
            if (rows) // k = 10 / 32 in rows of 4, else k and col at run time
                launch_fused_rows(F, B, *M, cd, slots, col);
            else
                launch_fused_out(F, B, *M, cd, slots, maxc);
        } else {
            launch_fused_flat(F, B, *M, maxc);
        }
        return (int)hipGetLastError();
    }
    if (cascade) {
        CascArgs A = {}; // (launch_cascade sets the lanes and the workspace)
        A.shards = sh, A.parity = pp;
        A.hdr_dw = reinterpret_cast<uint32_t*>(hdr), A.meta_dw = reinterpret_cast<const uint32_t*>(meta);
        A.fsize = fsize, A.present = present, A.parity_present = parity_present, A.recovered = recovered;
        casc_out_args(&A, out, stride, capacity);
        launch_cascade(A, *M, groups, cd, ws, B.rec_bytes, st,
                       !(flags & RFEC_KFLAG_MATRIX_GENERIC) && rfec_packed_matrix_col(&P));
        return (int)hipGetLastError();
    }
    RFEC_TAG(RFEC_PATH_PEEL_FLAT,
             (maxc <= 4 ? 4u : 8u) | (maxc <= 8 ? RFEC_PATH_FAST : 0u) | (dense ? RFEC_PATH_DENSE : 0u));
    launch_peel(B, *M, st);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess)
        return (int)e;
    launch_replay_flat(B, P, sh, pp, C, cd, maxc, DO, st);
    return (int)hipGetLastError();
}

} // namespace

extern "C" {

int rfec_timing_events(void* start, void* stop)
{
    t_ev_start = reinterpret_cast<hipEvent_t>(start);
    t_ev_stop = reinterpret_cast<hipEvent_t>(stop);
    t_launches = 0;
    return 0;
}

uint32_t rfec_timing_launches(void) { return t_launches; }

uint32_t rfec_last_path(void) { return t_path; }

uint32_t rfec_indexed_last_path(void) { return t_indexed_path; }

int rfec_launch_encode(const rfec_kplan* P, uint32_t groups, uint32_t stride, uint32_t capacity,
                       const uint8_t* shards, const rfec_hdr* hdr, uint8_t* parity, rfec_hdr* meta,
                       uint16_t* fsize, int8_t* status, void* stream, unsigned flags)
{
    uint32_t gpb = kMetaDwords / (5u * P->k);
    gpb = gpb < 1 ? 1 : (gpb > 64 ? 64 : gpb);
    if (gpb >= 4)
        gpb &= ~3u; // keeps every block's header slice 16-byte aligned
    const EncMeta E = {reinterpret_cast<const uint32_t*>(hdr), reinterpret_cast<uint32_t*>(meta), fsize, status, groups,
                       capacity, gpb, (groups + gpb - 1) / gpb};
    const uint32_t cd = capacity ? (capacity + 15) / 16 : 1;
    const EncLaunch a = {P, groups, stride, cd, reinterpret_cast<const v4u*>(shards), reinterpret_cast<v4u*>(parity),
                         E, reinterpret_cast<hipStream_t>(stream)};
    return (int)launch_encode(a, flags);
}

// rfec_recover_indexed_out (rfec_recover_indexed.c): rfec_recover_batch_out's dense decode with every member and
// parity row read through src_of from the pool `rows` [n_rows][stride].  Row layouts (rows of <= 4, k <= 64): one
// launch of k_decode_rows_indexed, no workspace.  Any other plan, and RFEC_KFLAG_GENERIC: k_peel_lds in dense mode
// (it reads the tables only), then k_recover_indexed.  n_rows == 0 (no slot can be present): the peel alone.
int rfec_launch_recover_indexed(const rfec_kmask* M, uint32_t groups, uint32_t stride, uint32_t capacity,
                                const uint8_t* rows, uint32_t n_rows, const uint32_t* src_of, const rfec_hdr* hdr,
                                const uint64_t* present, const rfec_hdr* meta, const uint16_t* fsize,
                                const uint64_t* parity_present, uint64_t* recovered, void* ws, void* stream,
                                unsigned flags, const rfec_dense_out* out)
{
    const rfec_kplan& P = M->plan;
    const uint32_t C = stride / 16, cd = capacity ? (capacity + 15) / 16 : 1, E = out ? out->per_group : 0;
    const uint32_t lg = rfec_header_lanes_log2(P.n_lines);
    if (!groups || !stride || stride % 16 || capacity > stride || !P.k || P.k > RFEC_MAX_K ||
        P.n_lines > RFEC_MAX_LINES || !E || E > P.k || (uint64_t)groups * E * cd >= (1ull << 31) ||
        ((uint64_t)groups << lg) >= (1ull << 32))
        return (int)hipErrorInvalidValue;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    PeelArgs B; // dense output: the header lanes and the peel only read hdr
    const PeelGeom G = peel_args(&B, *M, groups, capacity, const_cast<rfec_hdr*>(hdr), present, meta, fsize,
                                 parity_present, recovered, ws, out);
    const v4u* pool = reinterpret_cast<const v4u*>(rows);
    const uint32_t last = n_rows ? n_rows - 1 : 0;
    const DenseOut DO = {reinterpret_cast<v4u*>(out->shards), E};
    const uint32_t col = (uint32_t)rfec_rows_indexed_col(&P);
    if (n_rows && !(flags & RFEC_KFLAG_GENERIC) && col) {
        // launch_fused_rows' grid: header lanes per (group, line), payload lanes per (group, out slot, chunk)
        B.gpb = 1;
        B.nlp_log2 = lg;
        const FusedArgs F = {nullptr, nullptr, groups * cd, C, make_fastdiv(cd), blocks_for((uint64_t)groups << lg),
                             st, DO};
        t_indexed_path = 1u | (col == 4 && (P.k == 10 || P.k == 32) ? P.k : 0u) << 8;
        launch_rows_indexed(pool, last, src_of, F, B, *M, cd, col);
        return (int)hipGetLastError();
    }
    t_indexed_path = 2u | (G.maxc <= 4 ? 4u : 8u) << 8;
    launch_peel(B, *M, st);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess || !n_rows)
        return (int)e;
    launch_replay_indexed(B, P, pool, last, src_of, C, cd, G.maxc, DO, st);
    return (int)hipGetLastError();
}

int rfec_launch_recover(const rfec_kmask* M, uint32_t groups, uint32_t stride, uint32_t capacity,
                        uint8_t* shards, rfec_hdr* hdr, const uint64_t* present, const uint8_t* parity,
                        const rfec_hdr* meta, const uint16_t* fsize, const uint64_t* parity_present,
                        uint64_t* recovered, void* ws, void* stream, unsigned flags)
{
    return launch_recover(M, groups, stride, capacity, shards, hdr, present, parity, meta, fsize, parity_present,
                          recovered, ws, stream, flags, nullptr);
}

int rfec_launch_recover_out(const rfec_kmask* M, uint32_t groups, uint32_t stride, uint32_t capacity,
                            const uint8_t* shards, const rfec_hdr* hdr, const uint64_t* present,
                            const uint8_t* parity, const rfec_hdr* meta, const uint16_t* fsize,
                            const uint64_t* parity_present, uint64_t* recovered, void* ws, void* stream,
                            unsigned flags, const rfec_dense_out* out)
{
    // the fused decodes only read the shards and headers when the output is dense
    return launch_recover(M, groups, stride, capacity, const_cast<uint8_t*>(shards), const_cast<rfec_hdr*>(hdr),
                          present, parity, meta, fsize, parity_present, recovered, ws, stream, flags, out);
}

int rfec_rows_indexed_col(const rfec_kplan* P)
{
    uint32_t col = 0;
    return is_row_layout(P, &col) && col <= 4 && P->k <= 64 ? (int)col : 0;
}

int rfec_packed_matrix_col(const rfec_kplan* P)
{
    const uint32_t k = P->k, col = k <= 9 ? 3u : 4u;
    return k >= 6 && k <= 16 && is_full_matrix(P, col) ? (int)col : 0;
}

int rfec_full_matrix(const rfec_kplan* P, uint32_t col) { return col && is_full_matrix(P, col) ? 1 : 0; }

const char* rfec_hip_error_string(int code) { return hipGetErrorString((hipError_t)code); }

} // extern "C"
