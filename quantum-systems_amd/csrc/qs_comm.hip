// Multi-GPU entry points of the C ABI (include/qs_amd.h): an RCCL communicator behind an opaque handle and the
// four-index transform of a tensor sharded over the GPUs of one node, one process per GPU.
//
// The reference has no notion of a second device; SURVEY 8(b)/(e) asks for these entry points so that a
// host that is not Python can shard the path.  Layout (the one sharded.transform_two_body_sharded uses): `u` is
// sharded over its SECOND index (rank g holds u[:, b_lo:b_hi, :, :], balanced split), the result over its LEADING
// index (rank g gets out[p_lo:p_hi]).
//
//   local      d, c, then a (local in this layout):  X[p, b_loc, r, s] = Ct[p,a] u[a,b,c,d] C[c,r] C[d,s]
//   exchange   row p of X goes to the owner of p: (G-1)/G^2 of the tensor leaves every rank, one xGMI link per peer
//   close      out[p_loc][q, (r,s)] = Ct[q, b] R[p_loc][b, (r,s)]   with R[p_loc] = the rows received for p_loc
//
// RCCL is used directly: grouped ncclSend / ncclRecv pairs, one pair per row and peer, so that all seven links of a
// rank carry traffic at once (a ring all-to-all would be bound by one link).  The exchange is CHUNKED and runs on the
// communicator's own stream: the rows of Ct are taken in an order in which every chunk holds rows of EVERY peer;
// while chunk c travels, the contraction over a of chunk c + 1 and the closing contraction of chunk c - 1 run on the
// caller's stream.  No packing anywhere: a row of X is one contiguous message, and it lands at its final place
// R[p_loc][b_lo(sender) ...], from where the closing product reads it with K = L in one batched GEMM per chunk.
//
// RCCL is loaded at run time (dlopen of librccl.so.1: the copy PyTorch has already loaded when there is one), so the
// single-GPU library has no link-time dependency on it.

#include <dlfcn.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "qs_common.h"

namespace qs {

namespace {

// ---- the few RCCL symbols used, resolved once per process (the functions are process-wide facts, not state)
typedef void* nccl_comm_t;
struct NcclUniqueId { char internal[QS_UNIQUE_ID_BYTES]; };
typedef int (*fn_get_unique_id)(NcclUniqueId*);
typedef int (*fn_comm_init_rank)(nccl_comm_t*, int, NcclUniqueId, int);
typedef int (*fn_comm_destroy)(nccl_comm_t);
typedef int (*fn_comm_abort)(nccl_comm_t);
typedef int (*fn_group)(void);
typedef int (*fn_send)(const void*, size_t, int, int, nccl_comm_t, hipStream_t);
typedef int (*fn_recv)(void*, size_t, int, int, nccl_comm_t, hipStream_t);
typedef const char* (*fn_error_string)(int);
constexpr int kNcclFloat64 = 8;      // ncclFloat64 (rccl.h); complex128 travels as pairs of doubles

struct Rccl {
    void* handle = nullptr;
    fn_get_unique_id get_unique_id = nullptr;
    fn_comm_init_rank comm_init_rank = nullptr;
    fn_comm_destroy comm_destroy = nullptr;
    fn_comm_abort comm_abort = nullptr;      // optional
    fn_group group_start = nullptr, group_end = nullptr;
    fn_send send = nullptr;
    fn_recv recv = nullptr;
    fn_error_string error_string = nullptr;
    bool ok = false;
};

static thread_local char g_comm_err[256] = "";

const Rccl& rccl() {
    static const Rccl lib = [] {
        Rccl r;
        const char* names[] = {"librccl.so.1", "librccl.so"};
        // development / test hook: QS_AMD_RCCL_LIB names the library to load instead (the file-based stand-in of
        // tests/cabi/mock_rccl.cpp, which lets several ranks share one GPU, also inside a process that has PyTorch's RCCL)
        if (const char* forced = getenv("QS_AMD_RCCL_LIB")) {
            if (forced[0]) r.handle = dlopen(forced, RTLD_NOW | RTLD_LOCAL);
        }
        for (const char* n : names) {      // a copy that is already in the process (PyTorch's) first
            if (r.handle) break;
            r.handle = dlopen(n, RTLD_NOW | RTLD_NOLOAD);
        }
        for (const char* n : names) {
            if (r.handle) break;
            r.handle = dlopen(n, RTLD_NOW | RTLD_LOCAL);
        }
        if (!r.handle) return r;
        r.get_unique_id = (fn_get_unique_id)dlsym(r.handle, "ncclGetUniqueId");
        r.comm_init_rank = (fn_comm_init_rank)dlsym(r.handle, "ncclCommInitRank");
        r.comm_destroy = (fn_comm_destroy)dlsym(r.handle, "ncclCommDestroy");
        r.comm_abort = (fn_comm_abort)dlsym(r.handle, "ncclCommAbort");
        r.group_start = (fn_group)dlsym(r.handle, "ncclGroupStart");
        r.group_end = (fn_group)dlsym(r.handle, "ncclGroupEnd");
        r.send = (fn_send)dlsym(r.handle, "ncclSend");
        r.recv = (fn_recv)dlsym(r.handle, "ncclRecv");
        r.error_string = (fn_error_string)dlsym(r.handle, "ncclGetErrorString");
        r.ok = r.get_unique_id && r.comm_init_rank && r.comm_destroy && r.group_start && r.group_end && r.send &&
               r.recv && r.error_string;
        return r;
    }();
    return lib;
}

int rccl_status(int code, const char* what) {
    if (code == 0) return QS_OK;
    snprintf(g_comm_err, sizeof(g_comm_err), "%s: %s", what, rccl().error_string ? rccl().error_string(code) : "?");
    return QS_ERR_COMM;
}

constexpr int kMaxChunks = 16;

// balanced split of n rows over `world` ranks: the same rule as sharded.SlabPartition
inline int64_t part_lo(int64_t n, int world, int r) {
    const int64_t base = n / world, extra = n % world;
    return r * base + (r < extra ? r : extra);
}

// ---- one operation of an exchange step, the same for both entries.  It names the buffers its offsets refer to and the
// pitches of its copies, so that the executor (exchange_step) need not know which entry it serves.  The kinds, by the
// numbers the plan-export functions write and the CPU tests read: 0 a message out of the send block, 1 a message that
// lands in place in the result buffer, 2 this rank's own rows (strided copy send block -> result buffer), 3 a message
// into the staging area, 4 BEHIND the group: strided copy staging area -> result buffer.
enum OpKind { kSend, kRecv, kOwnRows, kRecvStaged, kUnstage };
enum Buf { kBufSend, kBufResult, kBufStage };
struct ExOp {
    int step, peer, kind;
    int64_t src_off, dst_off;         // element offsets into src_buf / dst_buf (0 on the side a message does not have)
    int64_t count, rows;              // a message of `count` elements; a copy of `rows` pieces of `count` elements ...
    int src_buf = kBufSend, dst_buf = kBufResult;
    int64_t src_pitch = 0, dst_pitch = 0;     // ... `src_pitch` / `dst_pitch` elements apart
};

// An `emit` that writes every op as a row of an exported plan (the plans as numbers let a CPU test replay every rank of a
// world with NumPy -- the part of this file that a one-GPU box cannot exercise with more than one rank).
struct TableWriter {
    int64_t* table;
    int64_t capacity, n;
    int operator()(const ExOp& o) {
        if (n >= capacity) return QS_ERR_WORKSPACE;
        const int64_t row[7] = {o.step, o.peer, o.kind, o.src_off, o.dst_off, o.count, o.rows};
        memcpy(table + 7 * n++, row, sizeof(row));
        return QS_OK;
    }
};

// ---- the plan of the slab entry: pure index arithmetic, shared by the entry and by qs_sharded_exchange_plan
struct SlabGeom {
    int G, me, nchunks;
    int64_t L, M, MM;
    int64_t b_lo, bl, p_lo, pc, row_x, row_r;       // row_x = bl*M*M elements of an X row, row_r = L*M*M of an R row
};

SlabGeom slab_geometry(int64_t L, int64_t M, int G, int me, int nchunks) {
    SlabGeom q;
    q.G = G; q.me = me; q.L = L; q.M = M; q.MM = M * M;
    q.nchunks = nchunks < 1 ? 4 : (nchunks > kMaxChunks ? kMaxChunks : nchunks);
    q.b_lo = part_lo(L, G, me); q.bl = part_lo(L, G, me + 1) - q.b_lo;
    q.p_lo = part_lo(M, G, me); q.pc = part_lo(M, G, me + 1) - q.p_lo;
    q.row_x = q.bl * q.MM; q.row_r = L * q.MM;
    return q;
}

// rows of chunk k that belong to peer g: [rows_lo(g, k), rows_lo(g, k + 1))
inline int64_t rows_lo(const SlabGeom& q, int g, int k) {
    const int64_t n = part_lo(q.M, q.G, g + 1) - part_lo(q.M, q.G, g);
    return part_lo(q.M, q.G, g) + part_lo(n, q.nchunks, k);
}

// X rows (in exchange order: chunk-major, then peer) of chunk k: [slab_slot0(k), slab_slot0(k + 1))
inline int64_t slab_slot0(const SlabGeom& q, int k) {
    int64_t slot = 0;
    for (int g = 0; g < q.G; ++g) slot += rows_lo(q, g, k) - rows_lo(q, g, 0);
    return slot;
}

// global row of Ct in X slot i, M entries
void slab_ct_rows(const SlabGeom& q, int64_t* ct_row) {
    int64_t slot = 0;
    for (int k = 0; k < q.nchunks; ++k)
        for (int g = 0; g < q.G; ++g)
            for (int64_t p = rows_lo(q, g, k); p < rows_lo(q, g, k + 1); ++p) ct_row[slot++] = p;
}

// The operations of chunk k, in the order both sides of every pair post them.  Our result rows that chunk k completes
// are [c_lo, c_lo + c_n) relative to p_lo.
template <typename F>
int slab_chunk_ops(const SlabGeom& q, int k, F&& emit) {
    const int64_t c_lo = rows_lo(q, q.me, k) - q.p_lo, c_n = rows_lo(q, q.me, k + 1) - rows_lo(q, q.me, k);
    int64_t slot = slab_slot0(q, k);
    for (int g = 0; g < q.G; ++g) {
        const int64_t n_send = rows_lo(q, g, k + 1) - rows_lo(q, g, k);
        const int64_t gb_lo = part_lo(q.L, q.G, g), gbl = part_lo(q.L, q.G, g + 1) - gb_lo;    // b range of rank g
        if (g == q.me) {
            // our own rows: straight into R (strided copy: a row of X is bl*MM long, a row of R is L*MM long)
            if (n_send > 0 && q.bl > 0)
                if (int rc = emit(ExOp{k, g, kOwnRows, slot * q.row_x, (c_lo * q.L + q.b_lo) * q.MM, q.row_x, n_send, kBufSend,
                                       kBufResult, q.row_x, q.row_r}))
                    return rc;
        } else {
            // what we computed for peer g goes out row by row; what peer g computed for us comes in row by row
            for (int64_t i = 0; i < n_send && q.bl > 0; ++i)
                if (int rc = emit(ExOp{k, g, kSend, (slot + i) * q.row_x, 0, q.row_x, 1})) return rc;
            for (int64_t i = 0; i < c_n && gbl > 0; ++i)
                if (int rc = emit(ExOp{k, g, kRecv, 0, ((c_lo + i) * q.L + gb_lo) * q.MM, gbl * q.MM, 1})) return rc;
        }
        slot += n_send;
    }
    return QS_OK;
}

// workspace of the slab entry, in elements: Ct rows in exchange order (at its start) | C^T | T1 (reused as X) | T2 | R
struct SlabLayout { int64_t CT, T1, T2, R, total; };
SlabLayout slab_layout(const SlabGeom& q) {
    const int64_t lm = (q.L * q.M + 1) & ~int64_t(1);
    const int64_t t1 = q.L * q.bl * q.L * q.M, x = q.M * q.row_x;
    SlabLayout w;
    w.CT = lm;                                // behind the rows of Ct in exchange order (chunk-major, then peer)
    w.T1 = w.CT + lm;                         // (L*bl*L, M); later X (M rows in exchange order) x (bl*M*M)
    w.T2 = w.T1 + (t1 > x ? t1 : x);          // (L*bl, M, M)
    w.R = w.T2 + q.L * q.row_x;               // (pc, L, M*M): row p_loc, columns b of every sender
    w.total = w.R + q.pc * q.row_r + 8;
    return w;
}

}  // namespace

struct Comm {
    nccl_comm_t nccl = nullptr;
    int rank = 0, world = 1, device = 0;
    hipStream_t stream = nullptr;              // the exchange runs here, beside the caller's stream
    hipEvent_t events[2 * kMaxChunks + 2] = {};      // (null until created: release() destroys what exists)
    hipEvent_t *x_ready = events, *r_ready = events + kMaxChunks, &idle = events[2 * kMaxChunks], &done = events[2 * kMaxChunks + 1];
    bool broken = false;                       // a call failed after its exchange had started: peers may be waiting in a
                                               // group this rank never completed -- only qs_comm_abort / destroy are left
    int rows_coalesce = 0;                     // qs_comm_set_option("rows_coalesce"): the rows exchange as ONE message per peer and step
};

// the end of a handle whose RCCL communicator is gone already: whatever of stream and events exists, then the struct
static void release(Comm* c) {
    for (hipEvent_t ev : c->events)
        if (ev) (void)hipEventDestroy(ev);
    if (c->stream) (void)hipStreamDestroy(c->stream);
    delete c;
}

// TEST HOOK (tuning key "comm_drop_wait", a bit mask, thread-local like every tuning key): leave out one of the waits
// that order the caller's stream and the communicator's stream.  The asynchronous stand-in transport of the test suite
// (tests/cabi/mock_rccl_async.cpp) must then produce WRONG results -- the proof that it would catch such a mistake.
//   1  rows: products of step t do not wait for the exchange of step t - 2 to have read their send block
//   2  rows: the exchange of a step does not wait for the step's products
//   4  rows: the closing products do not wait for the exchange
//   8  slab entry: the closing product of a chunk does not wait for the chunk's rows
//   16 slab entry: the exchange of a chunk does not wait for the chunk's products
inline bool dropped(int bit) { return (g_tune.comm_drop_wait & bit) != 0; }

// The entry checks that need the handle, in this order: it belongs to the caller's device and is not broken.
static int usable(const Comm* c) {
    if (current_device() != c->device) return QS_ERR_BAD_EXTENT;      // the communicator belongs to another device
    if (c->broken) {
        snprintf(g_comm_err, sizeof(g_comm_err), "the communicator was left broken by an earlier failed call: abort / destroy it");
        return QS_ERR_COMM;
    }
    return QS_OK;
}

// A failure of an entry.  `posted`: something of this call has been handed to RCCL (set by the first ncclGroupStart that
// succeeds), so the peers can be blocked in a group that this rank will never complete.  The handle is marked then, so
// that every later call fails at once instead of dead-locking too, and the caller tears the communicator down
// (qs_comm_abort).
static int failed(Comm* c, bool posted, int rc) {
    if (posted) c->broken = true;
    return rc;
}

// One exchange step of either entry.  The communicator's stream waits for what the caller's stream `s` has produced so
// far (x_ready[slot]; `wait_for_products` false only under the test hook above), then carries ONE group with the sends,
// receives and own-rows copies that `ops(emit)` emits, behind the group the copies out of the staging area, and last
// r_ready[slot].  base[Buf]: the three buffers the ops' offsets refer to, elements of `es` bytes.  The group is closed
// exactly once, also on an error.
template <typename Ops>
static int exchange_step(Comm* c, hipStream_t s, int slot, bool wait_for_products, void* const base[3], size_t es,
                         bool& posted, Ops&& ops) {
    hipError_t e = hipEventRecord(c->x_ready[slot], s);
    if (e == hipSuccess && wait_for_products) e = hipStreamWaitEvent(c->stream, c->x_ready[slot], 0);
    if (e != hipSuccess) return hip_status(e, "sharded exchange: chunk ready");
    if (int rc = rccl_status(rccl().group_start(), "ncclGroupStart")) return rc;
    posted = true;
    bool group_open = true;
    auto at = [&](int buf, int64_t elems) { return (void*)((char*)base[buf] + (size_t)elems * es); };
    const size_t width = es / sizeof(double);      // complex128 travels as pairs of doubles
    int rc = ops([&](const ExOp& o) -> int {
        if (o.kind == kSend)
            return rccl_status(rccl().send(at(o.src_buf, o.src_off), (size_t)o.count * width, kNcclFloat64, o.peer, c->nccl,
                                           c->stream), "ncclSend");
        if (o.kind == kRecv || o.kind == kRecvStaged)
            return rccl_status(rccl().recv(at(o.dst_buf, o.dst_off), (size_t)o.count * width, kNcclFloat64, o.peer, c->nccl,
                                           c->stream), "ncclRecv");
        if (o.kind == kUnstage && group_open) {      // (these follow every send / receive of the step)
            group_open = false;
            if (int grc = rccl_status(rccl().group_end(), "ncclGroupEnd")) return grc;
        }
        return hip_status(hipMemcpy2DAsync(at(o.dst_buf, o.dst_off), (size_t)o.dst_pitch * es, at(o.src_buf, o.src_off),
                                           (size_t)o.src_pitch * es, (size_t)o.count * es, (size_t)o.rows,
                                           hipMemcpyDeviceToDevice, c->stream), "sharded exchange: row copy");
    });
    if (group_open) {
        const int grc = rccl().group_end();
        if (!rc) rc = rccl_status(grc, "ncclGroupEnd");
    }
    if (rc) return rc;
    return hip_status(hipEventRecord(c->r_ready[slot], c->stream), "sharded exchange: rows ready");
}

}  // namespace qs

using namespace qs;

extern "C" {

const char* qs_last_comm_error(void) { return g_comm_err; }

int qs_comm_unique_id(void* id) {
    if (!id) return QS_ERR_NULL_POINTER;
    if (!rccl().ok) {
        snprintf(g_comm_err, sizeof(g_comm_err), "librccl.so.1 could not be loaded: %s", dlerror());
        return QS_ERR_COMM;
    }
    NcclUniqueId uid;
    if (int rc = rccl_status(rccl().get_unique_id(&uid), "ncclGetUniqueId")) return rc;
    memcpy(id, &uid, sizeof(uid));
    return QS_OK;
}

int qs_comm_init(void** comm, int rank, int world, const void* unique_id) {
    if (!comm || !unique_id) return QS_ERR_NULL_POINTER;
    if (world < 1 || rank < 0 || rank >= world) return QS_ERR_BAD_EXTENT;
    if (!rccl().ok) {
        snprintf(g_comm_err, sizeof(g_comm_err), "librccl.so.1 could not be loaded");
        return QS_ERR_COMM;
    }
    Comm* c = new Comm;
    c->rank = rank;
    c->world = world;
    c->device = current_device();
    NcclUniqueId uid;
    memcpy(&uid, unique_id, sizeof(uid));
    if (int rc = rccl_status(rccl().comm_init_rank(&c->nccl, world, uid, rank), "ncclCommInitRank")) { release(c); return rc; }
    hipError_t e = hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking);
    for (hipEvent_t& ev : c->events)
        if (e == hipSuccess) e = hipEventCreateWithFlags(&ev, hipEventDisableTiming);
    if (e != hipSuccess) {
        rccl().comm_destroy(c->nccl);
        release(c);
        return hip_status(e, "qs_comm_init: stream / events");
    }
    *comm = c;
    return QS_OK;
}

int qs_comm_destroy(void* comm) {
    if (!comm) return QS_ERR_NULL_POINTER;
    Comm* c = (Comm*)comm;
    (void)hipStreamSynchronize(c->stream);
    const int rc = rccl_status(rccl().comm_destroy(c->nccl), "ncclCommDestroy");
    release(c);
    return rc;
}

/* Tear a communicator down WITHOUT waiting for outstanding operations (ncclCommAbort): what is left to do after a call
 * returned an error in the middle of its exchange, or when a peer died.  Frees the handle. */
int qs_comm_abort(void* comm) {
    if (!comm) return QS_ERR_NULL_POINTER;
    Comm* c = (Comm*)comm;
    const int rc = rccl().comm_abort ? rccl_status(rccl().comm_abort(c->nccl), "ncclCommAbort")
                                     : rccl_status(rccl().comm_destroy(c->nccl), "ncclCommDestroy");
    release(c);
    return rc;
}

int qs_comm_rank(void* comm) { return comm ? ((Comm*)comm)->rank : QS_ERR_NULL_POINTER; }
int qs_comm_world(void* comm) { return comm ? ((Comm*)comm)->world : QS_ERR_NULL_POINTER; }

/* Exchange plan of one rank as numbers (no GPU, no RCCL): tests replay it on the CPU.  table: nops rows of
 * {chunk, peer, kind, x_off, r_off, count, rows}; header: {b_lo, bl, p_lo, pc, row_x, row_r, nchunks}; ct_rows: M;
 * chunks: per chunk {slot0, rows, close_lo, close_n}.  Returns the number of operations or a negative error. */
int qs_sharded_exchange_plan(int64_t L, int64_t M, int world, int rank, int nchunks, int64_t* header, int64_t* ct_rows,
                             int64_t* chunks, int64_t* table, int64_t table_rows) {
    if (L <= 0 || M <= 0 || M > 1024 || world < 1 || rank < 0 || rank >= world) return QS_ERR_BAD_EXTENT;
    if (!header || !ct_rows || !chunks || !table) return QS_ERR_NULL_POINTER;
    const SlabGeom q = slab_geometry(L, M, world, rank, nchunks);
    int64_t nops = 0;      // counted first: a table that is too small leaves every output as it was
    for (int k = 0; k < q.nchunks; ++k) slab_chunk_ops(q, k, [&](const ExOp&) { ++nops; return QS_OK; });
    if (nops > table_rows) return QS_ERR_WORKSPACE;
    const int64_t h[7] = {q.b_lo, q.bl, q.p_lo, q.pc, q.row_x, q.row_r, q.nchunks};
    memcpy(header, h, sizeof(h));
    slab_ct_rows(q, ct_rows);
    TableWriter row{table, table_rows, 0};
    for (int k = 0; k < q.nchunks; ++k) {
        chunks[4 * k] = slab_slot0(q, k);
        chunks[4 * k + 1] = slab_slot0(q, k + 1) - slab_slot0(q, k);
        chunks[4 * k + 2] = rows_lo(q, rank, k) - q.p_lo;
        chunks[4 * k + 3] = rows_lo(q, rank, k + 1) - rows_lo(q, rank, k);
        slab_chunk_ops(q, k, row);
    }
    return (int)row.n;
}

int64_t qs_transform_two_body_sharded_workspace(int dtype, int64_t L, int64_t M, int world, int rank) {
    if (!dtype_ok(dtype)) return QS_ERR_BAD_DTYPE;
    if (!extents_ok(L, M) || world < 1 || rank < 0 || rank >= world) return QS_ERR_BAD_EXTENT;
    return slab_layout(slab_geometry(L, M, world, rank, 0)).total * (int64_t)elem_size(dtype);
}

int qs_transform_two_body_sharded(void* comm, int dtype, const void* u_bslab, const void* C, const void* Ct,
                                  void* out_pslab, void* work, int64_t work_bytes, int64_t L, int64_t M, int nchunks,
                                  void* stream) {
    dispatch_reset();
    if (!comm) return QS_ERR_NULL_POINTER;
    Comm* c = (Comm*)comm;
    if (!dtype_ok(dtype)) return QS_ERR_BAD_DTYPE;
    if (!extents_ok(L, M)) return QS_ERR_BAD_EXTENT;
    if (!C || !Ct || !work) return QS_ERR_NULL_POINTER;
    const size_t es = elem_size(dtype);
    const SlabGeom q = slab_geometry(L, M, c->world, c->rank, nchunks);
    nchunks = q.nchunks;
    const int64_t bl = q.bl, MM = q.MM, row_x = q.row_x;
    if ((bl > 0 && !u_bslab) || (q.pc > 0 && !out_pslab)) return QS_ERR_NULL_POINTER;
    if (!aligned(C, es) || !aligned(Ct, es) || !aligned(work, 16) || (u_bslab && !aligned(u_bslab, es)) ||
        (out_pslab && !aligned(out_pslab, es)))
        return QS_ERR_MISALIGNED;
    if (out_pslab && (out_pslab == u_bslab || out_pslab == work)) return QS_ERR_ALIAS;
    const SlabLayout w = slab_layout(q);
    if (work_bytes < w.total * (int64_t)es) return QS_ERR_WORKSPACE;
    if (int rc = usable(c)) return rc;
    hipStream_t s = (hipStream_t)stream;

    auto at = [&](void* base, int64_t elems) { return (void*)((char*)base + (size_t)elems * es); };
    void *CtX = work, *CT = at(work, w.CT), *T1 = at(work, w.T1), *T2 = at(work, w.T2), *R = at(work, w.R);
    void* X = T1;

    // ---- Ct rows in exchange order (device-to-device row copies on the caller's stream: runs of consecutive rows)
    int64_t ct_row[1024];      // (extents_ok: M <= 1024)
    slab_ct_rows(q, ct_row);
    for (int64_t i = 0; i < M;) {
        int64_t n = 1;
        while (i + n < M && ct_row[i + n] == ct_row[i] + n) ++n;
        hipError_t ce = hipMemcpyAsync(at(CtX, i * L), (const char*)Ct + (size_t)(ct_row[i] * L) * es,
                                       (size_t)(n * L) * es, hipMemcpyDeviceToDevice, s);
        if (ce != hipSuccess) return hip_status(ce, "qs_transform_two_body_sharded: Ct rows");
        i += n;
    }
    int rc = QS_OK;
    if (bl > 0) {
        rc = transpose_small(dtype, C, CT, L, M, s);
        if (rc) return rc;
        // d:  T1[(a,b,c), s] = u[(a,b,c), d] C[d, s]
        rc = gemm(packed(dtype, u_bslab, C, T1, L * bl * L, M, L), s);
        if (rc) return rc;
        // c:  T2[(a,b)][r, s] = CT[r, c] T1[(a,b)][c, s]
        rc = gemm(packed(dtype, CT, T1, T2, M, M, L, L * bl), s);
        if (rc) return rc;
    }
    // the exchange must not start before earlier work on the caller's stream that R / X might still be read by
    hipError_t e = hipEventRecord(c->idle, s);
    if (e == hipSuccess) e = hipStreamWaitEvent(c->stream, c->idle, 0);
    if (e != hipSuccess) return hip_status(e, "qs_transform_two_body_sharded: stream order");

    auto close_chunk = [&](int k) -> int {
        // out[p][q, (r,s)] = Ct[q, :] . R[p][:, (r,s)] for our rows of chunk k, once they are complete
        const int64_t lo = rows_lo(q, q.me, k) - q.p_lo, n = rows_lo(q, q.me, k + 1) - rows_lo(q, q.me, k);
        if (n <= 0) return QS_OK;
        hipError_t ee = dropped(8) ? hipSuccess : hipStreamWaitEvent(s, c->r_ready[k], 0);
        if (ee != hipSuccess) return hip_status(ee, "qs_transform_two_body_sharded: wait for rows");
        return gemm(packed(dtype, Ct, at(R, lo * L * MM), at(out_pslab, lo * M * MM), M, MM, L, n), s);
    };
    void* const base[3] = {X, R, nullptr};
    bool posted = false;
    for (int k = 0; k < nchunks; ++k) {
        const int64_t slot0 = slab_slot0(q, k), rows_k = slab_slot0(q, k + 1) - slot0;
        // a:  X[slot, (b,r,s)] = CtX[slot, a] T2[a, (b,r,s)]   for the rows of chunk k
        if (bl > 0 && rows_k > 0) {
            rc = gemm(packed(dtype, at(CtX, slot0 * L), T2, at(X, slot0 * row_x), rows_k, row_x, L), s);
            if (rc) return failed(c, posted, rc);
        }
        // exchange of chunk k on the communicator's stream: one message per row and peer, all peers in one group
        rc = exchange_step(c, s, k, !dropped(16), base, es, posted, [&](auto&& emit) { return slab_chunk_ops(q, k, emit); });
        if (rc) return failed(c, posted, rc);
        // while chunk k travels: close chunk k - 1 (its rows have arrived or are about to)
        if (k > 0) { rc = close_chunk(k - 1); if (rc) return failed(c, posted, rc); }
    }
    rc = close_chunk(nchunks - 1);      // (the last group is closed: a failure from here on leaves no peer waiting)
    if (rc) return rc;
    // the caller's stream ends behind everything the exchange stream did (workspace and R are free after `stream`)
    e = hipEventRecord(c->done, c->stream);
    if (e == hipSuccess) e = hipStreamWaitEvent(s, c->done, 0);
    if (e != hipSuccess) return hip_status(e, "qs_transform_two_body_sharded: join");
    note_dispatch("rccl grouped send/recv (%d chunks)", nchunks);
    return QS_OK;
}

}  // extern "C"

// ------------------------------------------------------------------------------------------------------------------
// Rows in, rows out: the memory-lean form (what sharded.transform_two_body_rows does with torch.distributed, as ONE
// call on RCCL).  This rank holds rows[i][j][c][d], its rows i of ONE leading index of u with the other one whole
// (u[a_lo + i, j] for a leading-index sharding, u[j, b_lo + i] for a second-index sharding: the transform is symmetric
// under swapping its two leading index pairs), and gets the rows j' it owns of the OTHER transformed leading index,
// out[j'_loc][i'][r][s].  Apart from those two only O(chunk_rows * l^3) exists at any time:
//
//   per step of chunk_rows input rows, on the caller's stream:
//     d, c   t2[i][j][r, s] = C[c, r] rows[i][j][c, d] C[d, s]
//     J      W[j', i, (r,s)] = Ct[j', j] t2[i][j, (r,s)]         W is stored [j'][i][(r,s)]: a peer's share is one block
//   on the communicator's stream, overlapping the NEXT step's products (W is double-buffered):
//     grouped ncclSend / ncclRecv, one message per (peer, j'): n*M*M contiguous elements on both sides -- no packing,
//     no staging -- landing at R[j'_loc][i_global ...][(r,s)] inside the result buffer
//   after the last step, on the caller's stream, row by row inside the result buffer:
//     I      out[j'_loc][i', (r,s)] = Ct[i', i] R[j'_loc][i, (r,s)]
//
// Result rows are packed from the start of the buffer; received rows sit behind a gap of one row (plus the growth
// (M - L) M^2 per row when M > L), so the product of row p never reaches a received row that is still to be read.
// ------------------------------------------------------------------------------------------------------------------

namespace qs {
namespace {

constexpr int64_t kRowsBudgetBytes = int64_t(8) << 30;      // scratch per rank (as sharded.STREAM_BUDGET_BYTES)

struct RowsGeom {
    int G, me;
    int64_t L, M, MM, il, jl, il_max, i_start;      // my input rows [i_start, i_start + il), my result rows jl
    int64_t r0;                                     // element offset of received row 0 in the result buffer
    int64_t out_elems;
};

// start of rank g's input rows: the caller's table (world + 1 entries) or the balanced split
inline int64_t in_lo(const int64_t* in_starts, int64_t L, int G, int g) { return in_starts ? in_starts[g] : part_lo(L, G, g); }

int rows_geometry(RowsGeom& q, int64_t L, int64_t M, int G, int me, const int64_t* in_starts) {
    if (!extents_ok(L, M) || G < 1 || me < 0 || me >= G) return QS_ERR_BAD_EXTENT;
    if (in_starts) {
        if (in_starts[0] != 0 || in_starts[G] != L) return QS_ERR_BAD_EXTENT;
        for (int g = 0; g < G; ++g) if (in_starts[g + 1] < in_starts[g]) return QS_ERR_BAD_EXTENT;
    }
    q.G = G; q.me = me; q.L = L; q.M = M; q.MM = M * M;
    q.i_start = in_lo(in_starts, L, G, me);
    q.il = in_lo(in_starts, L, G, me + 1) - q.i_start;
    q.jl = part_lo(M, G, me + 1) - part_lo(M, G, me);
    q.il_max = 0;
    for (int g = 0; g < G; ++g) {
        const int64_t n = in_lo(in_starts, L, G, g + 1) - in_lo(in_starts, L, G, g);
        if (n > q.il_max) q.il_max = n;
    }
    q.r0 = q.jl * (M > L ? M - L : 0) * q.MM + L * q.MM;
    q.out_elems = q.jl * (M > L ? M : L) * q.MM + L * q.MM;
    return QS_OK;
}

inline int64_t clamp_rows(int64_t have, int64_t i0, int64_t ni) {
    const int64_t n = have - i0;
    return n < 0 ? 0 : (n > ni ? ni : n);
}

// The operations of one step, in the order both sides of every pair post them (peer ascending; per peer the sends in
// ascending j', the receives in ascending j'_loc): sends out of the step's send block W, receives into the result
// buffer, own rows W -> buffer (jl pieces of n*MM elements, pitches n*MM and L*MM).
// COALESCED form (one message per peer and step instead of one per peer and result row): a peer's share of W is one
// contiguous block anyway (W is stored [j'][i][(r,s)]), so its send has count = jc*n*MM; what the peer computed for us
// arrives as ONE block [j'_loc][i][(r,s)] in the staging area and is put in place by one strided copy on the
// communicator's stream behind the group (jl pieces of ng*MM elements, pitches ng*MM and L*MM).
template <typename F>
int rows_step_ops(const RowsGeom& q, const int64_t* in_starts, int64_t ni, int64_t step, bool coalesce, F&& emit) {
    const int64_t i0 = step * ni, n = clamp_rows(q.il, i0, ni), MM = q.MM;
    int64_t stage = 0;
    for (int g = 0; g < q.G; ++g) {
        const int64_t j_lo = part_lo(q.M, q.G, g), jc = part_lo(q.M, q.G, g + 1) - j_lo;
        const int64_t g_start = in_lo(in_starts, q.L, q.G, g);
        const int64_t ng = clamp_rows(in_lo(in_starts, q.L, q.G, g + 1) - g_start, i0, ni);   // rows rank g brings
        if (g == q.me) {
            if (n > 0 && q.jl > 0)
                if (int rc = emit(ExOp{(int)step, g, kOwnRows, j_lo * n * MM, q.r0 + (q.i_start + i0) * MM, n * MM, q.jl, kBufSend,
                                       kBufResult, n * MM, q.L * MM}))
                    return rc;
            continue;
        }
        if (coalesce) {
            if (jc > 0 && n > 0)
                if (int rc = emit(ExOp{(int)step, g, kSend, j_lo * n * MM, 0, jc * n * MM, 1})) return rc;
            if (q.jl > 0 && ng > 0) {
                if (int rc = emit(ExOp{(int)step, g, kRecvStaged, 0, stage, q.jl * ng * MM, 1, kBufSend, kBufStage})) return rc;
                stage += q.jl * ng * MM;
            }
            continue;
        }
        for (int64_t j = 0; j < jc && n > 0; ++j)
            if (int rc = emit(ExOp{(int)step, g, kSend, (j_lo + j) * n * MM, 0, n * MM, 1})) return rc;
        for (int64_t j = 0; j < q.jl && ng > 0; ++j)
            if (int rc = emit(ExOp{(int)step, g, kRecv, 0, q.r0 + (j * q.L + g_start + i0) * MM, ng * MM, 1})) return rc;
    }
    if (coalesce) {      // behind the group: the received blocks into place
        stage = 0;
        for (int g = 0; g < q.G; ++g) {
            if (g == q.me) continue;
            const int64_t g_start = in_lo(in_starts, q.L, q.G, g);
            const int64_t ng = clamp_rows(in_lo(in_starts, q.L, q.G, g + 1) - g_start, i0, ni);
            if (q.jl > 0 && ng > 0) {
                if (int rc = emit(ExOp{(int)step, g, kUnstage, stage, q.r0 + (g_start + i0) * MM, ng * MM, q.jl, kBufStage,
                                       kBufResult, ng * MM, q.L * MM}))
                    return rc;
                stage += q.jl * ng * MM;
            }
        }
    }
    return QS_OK;
}

// rows per step: the caller's chunk_rows (at most il_max), or for chunk_rows <= 0 the library's choice
inline int64_t rows_per_step(const RowsGeom& q, int64_t chunk_rows, size_t es) {
    if (chunk_rows >= 1) return chunk_rows > q.il_max ? q.il_max : chunk_rows;
    int64_t unit = q.L * q.L * q.M;
    if (q.L * q.MM > unit) unit = q.L * q.MM;
    if (q.M * q.MM > unit) unit = q.M * q.MM;
    int64_t ni = kRowsBudgetBytes / (5 * unit * (int64_t)es);
    const int64_t quarter = (q.il_max + 3) / 4;        // at least four steps, so that the exchange has products to hide under
    if (ni > quarter) ni = quarter;
    return ni < 1 ? 1 : ni;
}

// workspace of the rows entry, in elements: C^T (at its start) | t1 | t2 | W0 | W1 | S.  S, the staging area of the coalesced exchange,
// is empty without the option "rows_coalesce" of handle `c` (and without a handle); with it, what the peers send this rank
// in one step: jl (world - 1) blocks of at most ni*M*M elements, about one more send block.
struct RowsLayout { int64_t T1, T2, W[2], S, total; };
RowsLayout rows_layout(int64_t L, int64_t M, int64_t ni, const Comm* c) {
    const int64_t lm = (L * M + 1) & ~int64_t(1), MM = M * M;
    const int64_t staged = c && c->rows_coalesce ? (part_lo(M, c->world, c->rank + 1) - part_lo(M, c->world, c->rank)) * (c->world - 1) : 0;
    RowsLayout w;
    w.T1 = lm;
    w.T2 = w.T1 + ni * L * L * M;
    w.W[0] = w.T2 + ni * L * MM;
    w.W[1] = w.W[0] + M * ni * MM;
    w.S = w.W[1] + M * ni * MM;
    w.total = w.S + staged * ni * MM + 8;
    return w;
}
int64_t rows_workspace_bytes(int dtype, int64_t L, int64_t M, int64_t chunk_rows, const Comm* c) {
    if (!dtype_ok(dtype)) return QS_ERR_BAD_DTYPE;
    if (!extents_ok(L, M) || chunk_rows < 1 || chunk_rows > L) return QS_ERR_BAD_EXTENT;
    return rows_layout(L, M, chunk_rows, c).total * (int64_t)elem_size(dtype);
}

}  // namespace
}  // namespace qs

extern "C" {

/* chunk_rows the library picks when the caller passes <= 0 (a function of the GLOBAL extents only: every rank gets
 * the same number) */
int64_t qs_sharded_rows_default_chunk(int dtype, int64_t L, int64_t M, int world, const int64_t* in_starts) {
    if (!dtype_ok(dtype)) return QS_ERR_BAD_DTYPE;
    RowsGeom q;
    if (int rc = rows_geometry(q, L, M, world, 0, in_starts)) return rc;
    return rows_per_step(q, 0, elem_size(dtype));
}

/* bytes of the result buffer (the result rows are its first jl * M^3 elements) */
int64_t qs_transform_two_body_sharded_rows_out_bytes(int dtype, int64_t L, int64_t M, int world, int rank) {
    if (!dtype_ok(dtype)) return QS_ERR_BAD_DTYPE;
    RowsGeom q;
    if (int rc = rows_geometry(q, L, M, world, rank, nullptr)) return rc;
    return q.out_elems * (int64_t)elem_size(dtype);
}

int64_t qs_transform_two_body_sharded_rows_workspace(int dtype, int64_t L, int64_t M, int64_t chunk_rows) {
    return rows_workspace_bytes(dtype, L, M, chunk_rows, nullptr);
}

/* ... for THIS handle: with the option "rows_coalesce" the staging area of the coalesced exchange follows */
int64_t qs_comm_rows_workspace(void* comm, int dtype, int64_t L, int64_t M, int64_t chunk_rows) {
    if (!comm) return QS_ERR_NULL_POINTER;
    return rows_workspace_bytes(dtype, L, M, chunk_rows, (const Comm*)comm);
}

/* Per-handle options.  "rows_coalesce" = 1: qs_transform_two_body_sharded_rows exchanges ONE message per peer and step
 * (the peer's block of the send buffer as it is; the received block goes through a staging area of the workspace and is
 * put in place by one strided copy on the communicator's stream) instead of one message per peer and result row that
 * lands in place.  Same results bit for bit; every rank of the communicator must choose the same. */
int qs_comm_set_option(void* comm, const char* key, int64_t value) {
    if (!comm || !key) return QS_ERR_NULL_POINTER;
    Comm* c = (Comm*)comm;
    if (!strcmp(key, "rows_coalesce")) { c->rows_coalesce = value != 0; return QS_OK; }
    return QS_ERR_BAD_EXTENT;
}

/* The exchange plan of one rank as numbers (no GPU, no RCCL): the CPU suite replays the plans of every rank of a world
 * with NumPy.  header: {i_start, il, jl, il_max, r0, out_elems, chunk_rows, nsteps}; table: one row
 * {step, peer, kind, w_off, buf_off, count, rows} per operation.  Returns the number of operations or an error. */
static int rows_exchange_plan(int64_t L, int64_t M, int world, int rank, const int64_t* in_starts, int64_t chunk_rows,
                              bool coalesce, int64_t* header, int64_t* table, int64_t table_rows) {
    if (!header || !table) return QS_ERR_NULL_POINTER;
    RowsGeom q;
    if (int rc = rows_geometry(q, L, M, world, rank, in_starts)) return rc;
    const int64_t ni = rows_per_step(q, chunk_rows, 8);
    const int64_t nsteps = (q.il_max + ni - 1) / ni;
    const int64_t h[8] = {q.i_start, q.il, q.jl, q.il_max, q.r0, q.out_elems, ni, nsteps};
    memcpy(header, h, sizeof(h));
    TableWriter row{table, table_rows, 0};
    for (int64_t t = 0; t < nsteps; ++t)
        if (int rc = rows_step_ops(q, in_starts, ni, t, coalesce, row)) return rc;
    return (int)row.n;
}

int qs_sharded_rows_exchange_plan(int64_t L, int64_t M, int world, int rank, const int64_t* in_starts, int64_t chunk_rows,
                                  int64_t* header, int64_t* table, int64_t table_rows) {
    return rows_exchange_plan(L, M, world, rank, in_starts, chunk_rows, false, header, table, table_rows);
}

/* ... of the coalesced exchange (qs_comm_set_option "rows_coalesce"): kind 0 send (one per peer), 3 receive into the
 * staging area (buf_off = offset into it), 4 staging -> out_buffer behind the group (w_off = offset into the staging
 * area, `rows` pieces of `count` elements, pitches count and L*M*M), 2 own rows as before. */
int qs_sharded_rows_exchange_plan_coalesced(int64_t L, int64_t M, int world, int rank, const int64_t* in_starts,
                                            int64_t chunk_rows, int64_t* header, int64_t* table, int64_t table_rows) {
    return rows_exchange_plan(L, M, world, rank, in_starts, chunk_rows, true, header, table, table_rows);
}

int qs_transform_two_body_sharded_rows(void* comm, int in_dtype, int dtype, const void* rows, const int64_t* in_starts,
                                       const void* C, const void* Ct, void* out_buffer, int64_t out_bytes, void* work,
                                       int64_t work_bytes, int64_t L, int64_t M, int64_t chunk_rows, void* stream) {
    dispatch_reset();
    if (!comm) return QS_ERR_NULL_POINTER;
    Comm* c = (Comm*)comm;
    if (!dtype_ok(dtype) || !dtype_ok(in_dtype) || (in_dtype == QS_C128 && dtype == QS_F64)) return QS_ERR_BAD_DTYPE;
    RowsGeom q;
    if (int rc = rows_geometry(q, L, M, c->world, c->rank, in_starts)) return rc;
    if (!C || !Ct || !work || !out_buffer) return QS_ERR_NULL_POINTER;
    if (q.il > 0 && !rows) return QS_ERR_NULL_POINTER;
    const size_t es = elem_size(dtype), ies = elem_size(in_dtype);
    if (!aligned(C, es) || !aligned(Ct, es) || !aligned(work, 16) || !aligned(out_buffer, 16) || (rows && !aligned(rows, ies)))
        return QS_ERR_MISALIGNED;
    if (out_buffer == rows || out_buffer == work) return QS_ERR_ALIAS;
    const int64_t ni = rows_per_step(q, chunk_rows, es);
    const RowsLayout w = rows_layout(L, M, ni, c);
    if (out_bytes < q.out_elems * (int64_t)es) return QS_ERR_WORKSPACE;
    if (work_bytes < w.total * (int64_t)es) return QS_ERR_WORKSPACE;
    if (int rc = usable(c)) return rc;
    hipStream_t s = (hipStream_t)stream;
    const int64_t MM = q.MM;
    const int64_t nsteps = (q.il_max + ni - 1) / ni;

    auto at = [&](void* base, int64_t elems) { return (void*)((char*)base + (size_t)elems * es); };
    void *CT = work, *T1 = at(work, w.T1), *T2 = at(work, w.T2);
    const bool coalesce = c->rows_coalesce != 0;
    bool posted = false;

    int rc = transpose_small(dtype, C, CT, L, M, s);
    if (rc) return rc;
    for (int64_t t = 0; t < nsteps; ++t) {
        const int slot = (int)(t & 1);                   // W is double-buffered, and so are the step's two events
        const int64_t i0 = t * ni, n = clamp_rows(q.il, i0, ni);
        void* const base[3] = {at(work, w.W[slot]), out_buffer, at(work, w.S)};
        hipError_t e = hipSuccess;
        // the send block was last read by the exchange of step t - 2
        if (t >= 2 && !dropped(1)) e = hipStreamWaitEvent(s, c->r_ready[slot], 0);
        if (e != hipSuccess) return failed(c, posted, hip_status(e, "qs_transform_two_body_sharded_rows: send buffer free"));
        if (n > 0) {
            const void* src = (const char*)rows + (size_t)(i0 * L * L * L) * ies;
            // d:  t1[(i,j,c), s] = rows[(i,j,c), d] C[d, s]        (a real tensor against complex coefficients: the mixed product)
            rc = gemm_d(in_dtype, dtype, src, C, T1, n * L * L, L, M, s);
            if (rc) return failed(c, posted, rc);
            // c:  t2[(i,j)][r, s] = CT[r, c] t1[(i,j)][c, s]
            rc = gemm(packed(dtype, CT, T1, T2, M, M, L, n * L), s);
            if (rc) return failed(c, posted, rc);
            // J:  W[j', i, (r,s)] = Ct[j', j] t2[i][j, (r,s)]     one product per row i, rows of W n*MM apart: the packed form
            // of batch n but for W's row pitch and batch stride
            Product J = packed(dtype, Ct, T2, base[kBufSend], M, MM, L, n);
            J.ldc = n * MM;
            J.sc = MM;
            rc = gemm(J, s);
            if (rc) return failed(c, posted, rc);
        }
        rc = exchange_step(c, s, slot, !dropped(2), base, es, posted,
                           [&](auto&& emit) { return rows_step_ops(q, in_starts, ni, t, coalesce, emit); });
        if (rc) return failed(c, posted, rc);
    }
    // every received row is complete only now: the closing products follow the whole exchange
    hipError_t e = hipEventRecord(c->done, c->stream);
    if (e == hipSuccess && !dropped(4)) e = hipStreamWaitEvent(s, c->done, 0);
    if (e != hipSuccess) return failed(c, posted, hip_status(e, "qs_transform_two_body_sharded_rows: join"));
    // I:  out[p][i', (r,s)] = Ct[i', i] R[p][i, (r,s)], row by row, packed from the start of the buffer
    // (the last group is closed: a failure from here on leaves no peer waiting)
    for (int64_t p = 0; p < q.jl; ++p) {
        rc = gemm(packed(dtype, Ct, at(out_buffer, q.r0 + p * L * MM), at(out_buffer, p * M * MM), M, MM, L), s);
        if (rc) return rc;
    }
    note_dispatch("rccl grouped send/recv (%lld steps of %lld rows%s)", (long long)nsteps, (long long)ni,
                  coalesce ? ", one message per peer and step" : "");
    return QS_OK;
}

}  // extern "C"
