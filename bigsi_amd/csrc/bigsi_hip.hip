// bigsi_hip.hip -- host side of libbigsi_hip.so: the C ABI declared in include/bigsi_hip.h.
// Plain HIP runtime (hipMalloc / streams / events); no torch types anywhere in this library.
#include "bigsi_internal.hpp"

#include <algorithm>
#include <atomic>
#include <cerrno>
#include <chrono>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>
#include <string>
#include <thread>
#include <vector>

#include "bigsi_kernels.hpp"

using namespace bigsi;

// ------------------------------------------------------------------------------ errors
static thread_local char g_err[1024] = "";

int bigsi_fail(int code, const char *fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof g_err, fmt, ap);
    va_end(ap);
    return code;
}

extern "C" const char *bigsi_hip_last_error(void) { return g_err; }

extern "C" int bigsi_hip_device_count(int *out)
{
    if (!out) return fail(BIGSI_ERR_INVALID, "out is NULL");
    HIP_TRY(hipGetDeviceCount(out));
    return BIGSI_OK;
}

int bigsi_use_device(const bigsi_hip_index *ix)
{
    int cur = -1;
    if (hipGetDevice(&cur) == hipSuccess && cur == ix->device) return BIGSI_OK;      // (a thread-local read: every entry point comes through here)
    HIP_TRY(hipSetDevice(ix->device));
    return BIGSI_OK;
}
#define use_device bigsi_use_device

// The one-launch read kernel (k_reads_fused) of successive batches goes out on alternating library streams, so that one
// batch's k-merising and hit compaction -- phases with the HBM idle -- overlap the row fetches of its neighbours (BASELINE
// configs[1]: 31.6 -> 25 us per step).  Ordering: a batch's next run waits for its own `done` event; everything that
// changes the index, reads the profiling events or hands the stream back waits for the read streams (quiesce_reads).
static int read_stream(bigsi_hip_index *ix, hipStream_t *out)
{
    *out = ix->stream;
    if (ix->stream != ix->own_stream) return BIGSI_OK;       // the caller's own stream (bigsi_hip_set_stream): everything stays on it
    if (!ix->rd_stream[0])
        for (auto &st : ix->rd_stream) HIP_TRY(hipStreamCreateWithFlags(&st, hipStreamNonBlocking));
    *out = ix->rd_stream[ix->rd_next++ % (uint32_t)kReadStreamsUsed];
    ix->rd_pending = true;
    return BIGSI_OK;
}

// end of a batch run on the index stream: what later read-kernel launches wait for.  Only once read streams exist (an index
// that serves gene-length queries alone never pays for the record).
static int mark_main(bigsi_hip_index *ix)
{
    if (!ix->rd_stream[0] || ix->stream != ix->own_stream) return BIGSI_OK;
    if (!ix->main_ev) HIP_TRY(hipEventCreateWithFlags(&ix->main_ev, hipEventDisableTiming));
    HIP_TRY(hipEventRecord(ix->main_ev, ix->stream));
    return BIGSI_OK;
}

// K5 / K6 (scored searches) run on a stream of their own with the HIGHEST priority: they are a few small kernels whose result
// the host waits for while the NEXT batch's row-AND kernel fills the device, and at equal priority their workgroups queue up
// behind that kernel's (bench workload c5: 0.37 ms of waiting for 0.05 ms of work).  A request may stay queued here after its
// _begin returns (sc_pending): calls that change the index wait for it (quiesce_index).
static int score_stream(bigsi_hip_index *ix, hipStream_t *out)
{
    *out = ix->stream;
    if (ix->stream != ix->own_stream) return BIGSI_OK;       // the caller's own stream: everything stays on it
    if (!ix->sc_stream) {
        int least = 0, greatest = 0;
        HIP_TRY(hipDeviceGetStreamPriorityRange(&least, &greatest));
        HIP_TRY(hipStreamCreateWithPriority(&ix->sc_stream, hipStreamNonBlocking, greatest));
    }
    *out = ix->sc_stream;
    return BIGSI_OK;
}

static int quiesce_reads(bigsi_hip_index *ix)
{
    if (!ix->rd_pending) return BIGSI_OK;
    for (auto st : ix->rd_stream)
        if (st) HIP_TRY(hipStreamSynchronize(st));
    ix->rd_pending = false;
    return BIGSI_OK;
}

// Everything that reads the matrix on a stream other than the index stream is over: the read streams AND the score stream
// (a K5 request between its _begin and its _end -- bigsi_hip_batch_score_hits_begin, the scored stream's chunks -- is
// k_presence_bits reading d_index there).  Every entry point that changes the index, hands the stream back or reads the
// profiling events calls this; batch runs call quiesce_reads only (scoring beside the next batch's row-AND is the point).
static int quiesce_index(bigsi_hip_index *ix)
{
    TRY(quiesce_reads(ix));
    if (ix->sc_pending && ix->sc_stream) HIP_TRY(hipStreamSynchronize(ix->sc_stream));
    ix->sc_pending = false;
    return BIGSI_OK;
}

static uint64_t stride_for(uint64_t cols)
{
    return std::max<uint64_t>(16, round_up(ceil_div(cols, 64), 16));
}

// ------------------------------------------------------------------------------ lifecycle
int bigsi_writable(const bigsi_hip_index *ix)
{
    if (ix && ix->attach != bigsi_hip_index::kOwner)
        return fail(BIGSI_ERR_STATE, "this handle does not own its matrix (%s): it is read-only", ix->attach == bigsi_hip_index::kIpc ? "attached over hipIpc" : "a view");
    return BIGSI_OK;
}

// ------------------------------------------------------------------------------ shared guards of the calls that change an index
// What a call that rewrites a matrix in place needs before it touches it (compact_columns, fold_rows, shrink_to_fit, trim_rows and a
// reserve_cols that re-strides): the handle owns the matrix, no view of it is open (`stale`: what would happen to the views), its device
// is current and nothing reads the matrix on another stream.  A call's no-op returns come before this: a view may ask for nothing.
static int begin_rewrite(bigsi_hip_index *ix, const char *who, const char *stale)
{
    TRY(bigsi_writable(ix));
    if (ix->views.load() > 0) return fail(BIGSI_ERR_STATE, "%s: %d view(s) of this index are open: %s", who, ix->views.load(), stale);
    TRY(use_device(ix));
    return quiesce_index(ix);
}

// The matrix moves to an allocation of its own size, num_rows rows of `new_stride` words: through k_restride when the stride changes
// (min(old, new) words of every row, zeros behind them), as one device-to-device copy of the front of the old allocation when it
// does not (bigsi_hip_trim_rows).  The second matrix has to fit beside the first (BIGSI_ERR_NOMEM); on any failure the index is as it
// was, nothing is leaked and the runtime's sticky last-error slot is clear for this thread's next launch check.
static int replace_matrix(bigsi_hip_index *ix, uint64_t new_stride, const char *who)
{
    const size_t bytes = (size_t)ix->m * new_stride * 8;
    uint64_t *nd = nullptr;
    hipError_t e = hipMalloc((void **)&nd, bytes);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        return fail(e == hipErrorOutOfMemory ? BIGSI_ERR_NOMEM : BIGSI_ERR_HIP, "%s: hipMalloc of %zu bytes beside the matrix failed: %s", who, bytes,
                    hipGetErrorString(e));
    }
    if (new_stride != ix->stride_words) {
        const unsigned grid = (unsigned)std::min<uint64_t>(ceil_div(ix->m * new_stride, kBlock), 256 * 8 * 4);
        hipLaunchKernelGGL(k_restride, dim3(grid), dim3(kBlock), 0, ix->stream, ix->d_index, ix->stride_words, nd, new_stride, ix->m);
        e = hipGetLastError();
    } else
        e = hipMemcpyAsync(nd, ix->d_index, bytes, hipMemcpyDeviceToDevice, ix->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(ix->stream);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        hipError_t e2 = hipFree(nd); (void)e2;
        return fail(BIGSI_ERR_HIP, "%s: copying the rows failed: %s", who, hipGetErrorString(e));
    }
    HIP_TRY(hipFree(ix->d_index));
    ix->d_index = nd;
    ix->alloc_rows = ix->m;          // (the new allocation holds the rows the index has: what a fold left behind them is gone)
    ix->stride_words = new_stride;
    ix->cap_cols = new_stride * 64;
    return BIGSI_OK;
}

// The calls that make or grow one index from another (extract_columns, fold_rows_into, collapse_columns_into, append_index): what the
// two handles must have in common, checked in one order for all of them.  An entry point checks its own arguments before this.
namespace {
struct DeriveRule {
    const char *name;          // the entry point, for messages
    const char *in_place;      // the in-place form a caller may have meant, or nullptr: there is none
    bool rows_divide;          // the destination's num_rows divides the source's (a fold); otherwise the two are equal
    bool same_hashes;          // num_hashes must match
    bool into_empty;           // the destination holds no columns and has no views open (append_index grows it, as insert_columns does)
};
}  // namespace

static int check_derive(const DeriveRule &r, const bigsi_hip_index *dst, const bigsi_hip_index *src)
{
    if (!dst || !src) return fail(BIGSI_ERR_INVALID, "NULL argument");
    const std::string hint = r.in_place ? std::string(r.in_place) + " works in place" : std::string("there is no in-place form");
    if (dst == src) return fail(BIGSI_ERR_INVALID, "%s: dst and src are the same index (%s)", r.name, hint.c_str());
    if (r.rows_divide ? (dst->m == 0 || src->m % dst->m) : dst->m != src->m)
        return fail(BIGSI_ERR_INVALID, r.rows_divide ? "the destination's num_rows %llu does not divide the source's %llu" : "row counts differ (%llu vs %llu)",
                    (unsigned long long)dst->m, (unsigned long long)src->m);
    if (dst->device != src->device) return fail(BIGSI_ERR_INVALID, "both indexes must live on the same device");
    if (r.same_hashes && dst->h != src->h) return fail(BIGSI_ERR_INVALID, "num_hashes differ (%u vs %u)", dst->h, src->h);
    TRY(bigsi_writable(dst));
    if (dst->d_index == src->d_index) return fail(BIGSI_ERR_INVALID, "%s: src is a view of dst (%s)", r.name, hint.c_str());
    if (!r.into_empty) return BIGSI_OK;
    if (dst->views.load() > 0)
        return fail(BIGSI_ERR_STATE, "%s: %d view(s) of the destination are open: their column count would go stale", r.name, dst->views.load());
    if (dst->n_cols != 0) return fail(BIGSI_ERR_STATE, "%s: the destination already holds %llu column(s)", r.name, (unsigned long long)dst->n_cols);
    return BIGSI_OK;
}

// Both handles are held for the whole call: the source's matrix must not be re-strided, folded, compacted or closed by another host
// thread under the kernel that reads it.
#define BIGSI_ENTER_DERIVE(dstp, srcp)                                                                                             \
    BIGSI_ENTER(dstp);                                                                                                             \
    BusyGuard src_guard_(srcp);                                                                                                    \
    if (!src_guard_.ok)                                                                                                            \
        return fail(BIGSI_ERR_STATE, "the source index handle is in use by another host thread (one handle = one thread at a time)")

// ... and what they do once the checks are through: room for `cols` columns in the destination, nothing reading it on another
// stream, and the source's stream drained (streams of different handles are not ordered with each other)
static int begin_derive(bigsi_hip_index *dst, const bigsi_hip_index *src, uint64_t cols)
{
    TRY(bigsi_hip_reserve_cols(dst, cols));
    TRY(use_device(dst));
    TRY(quiesce_index(dst));
    HIP_TRY(hipStreamSynchronize(src->stream));
    return BIGSI_OK;
}

// the matrix of a new handle: allocated and zeroed here (ipc == nullptr && view == nullptr), another process's allocation mapped
// into this one (ipc), or another handle's pointer (view)
static int open_impl(uint64_t num_rows, uint64_t num_cols, uint64_t col_capacity, uint32_t num_hashes, int device, const hipIpcMemHandle_t *ipc,
                     const bigsi_hip_index *view, bigsi_hip_index **out)
{
    if (!out) return fail(BIGSI_ERR_INVALID, "out is NULL");
    *out = nullptr;
    if (num_rows == 0) return fail(BIGSI_ERR_INVALID, "num_rows must be > 0");
    if (num_hashes == 0) return fail(BIGSI_ERR_INVALID, "num_hashes must be > 0");
    if (col_capacity < num_cols) col_capacity = num_cols;
    if (col_capacity == 0) col_capacity = 64;
    if (col_capacity > 0xFFFFFFFFull) return fail(BIGSI_ERR_INVALID, "col_capacity %llu exceeds 2^32-1 colours per shard", (unsigned long long)col_capacity);
    int ndev = 0;
    HIP_TRY(hipGetDeviceCount(&ndev));
    if (device < 0 || device >= ndev) return fail(BIGSI_ERR_INVALID, "device %d not in [0,%d)", device, ndev);
    HIP_TRY(hipSetDevice(device));
    bigsi_hip_index *ix = new (std::nothrow) bigsi_hip_index();
    if (!ix) return fail(BIGSI_ERR_NOMEM, "host allocation failed");
    ix->device = device;
    ix->m = num_rows;
    ix->alloc_rows = num_rows;
    ix->n_cols = num_cols;
    ix->h = num_hashes;
    ix->stride_words = stride_for(col_capacity);
    ix->cap_cols = ix->stride_words * 64;
    hipError_t e = hipStreamCreateWithFlags(&ix->own_stream, hipStreamNonBlocking);
    if (e != hipSuccess) { delete ix; return fail(BIGSI_ERR_HIP, "hipStreamCreate: %s", hipGetErrorString(e)); }
    ix->stream = ix->own_stream;
    {
        // lowest priority: whatever runs here must not delay the workgroups of a row-AND kernel on the index stream
        int least = 0, greatest = 0;
        e = hipDeviceGetStreamPriorityRange(&least, &greatest);
        if (e == hipSuccess) e = hipStreamCreateWithPriority(&ix->pre_stream, hipStreamNonBlocking, least);
        else e = hipStreamCreateWithFlags(&ix->pre_stream, hipStreamNonBlocking);
    }
    if (e != hipSuccess) {
        hipError_t e2 = hipStreamDestroy(ix->own_stream); (void)e2;
        delete ix;
        return fail(BIGSI_ERR_HIP, "hipStreamCreate: %s", hipGetErrorString(e));
    }
    const size_t bytes = (size_t)ix->m * ix->stride_words * 8;
    if (view) {
        ix->d_index = view->d_index;
        ix->attach = bigsi_hip_index::kView;
        ix->view_of = const_cast<bigsi_hip_index *>(view);
        ix->view_of->views++;
        *out = ix;
        return BIGSI_OK;
    }
    if (ipc) {
        void *p = nullptr;
        e = hipIpcOpenMemHandle(&p, *ipc, hipIpcMemLazyEnablePeerAccess);
        if (e != hipSuccess) {
            (void)hipGetLastError();          // (the runtime's last-error slot is sticky: the next launch check of this thread must not inherit it)
            hipError_t e2 = hipStreamDestroy(ix->own_stream); (void)e2;
            e2 = hipStreamDestroy(ix->pre_stream);
            delete ix;
            return fail(BIGSI_ERR_HIP, "hipIpcOpenMemHandle: %s (the owner must be another live process on this device; HSA_ENABLE_IPC_MODE_LEGACY=0 on hosts whose "
                                       "driver only does dmabuf IPC)", hipGetErrorString(e));
        }
        ix->d_index = static_cast<uint64_t *>(p);
        ix->attach = bigsi_hip_index::kIpc;
        *out = ix;
        return BIGSI_OK;
    }
    e = hipMalloc((void **)&ix->d_index, bytes);
    if (e != hipSuccess) {
        hipError_t e2 = hipStreamDestroy(ix->own_stream); (void)e2;
        e2 = hipStreamDestroy(ix->pre_stream);
        delete ix;
        return fail(BIGSI_ERR_NOMEM, "hipMalloc of %zu index bytes failed: %s", bytes, hipGetErrorString(e));
    }
    e = hipMemsetAsync(ix->d_index, 0, bytes, ix->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(ix->stream);
    if (e != hipSuccess) {
        hipError_t e2 = hipFree(ix->d_index); (void)e2;
        e2 = hipStreamDestroy(ix->own_stream);
        e2 = hipStreamDestroy(ix->pre_stream);
        delete ix;
        return fail(BIGSI_ERR_HIP, "zeroing the index failed: %s", hipGetErrorString(e));
    }
    *out = ix;
    return BIGSI_OK;
}

extern "C" int bigsi_hip_open(uint64_t num_rows, uint64_t num_cols, uint64_t col_capacity, uint32_t num_hashes, int device,
                              bigsi_hip_index **out)
{
    return open_impl(num_rows, num_cols, col_capacity, num_hashes, device, nullptr, nullptr, out);
}

// ------------------------------------------------------------------------------ an index shared between processes / threads
// The reference opens its store once per request and once per pool worker (bigsi/__main__.py:75-80, 204-205;
// storage/berkeleydb.py:12-19): the data lives in a file, any process can open it.  Here the data lives in ONE process's HBM
// allocation; these three give other handles onto it without a second copy:
//   export_ipc   the owner's matrix as a 64-byte hipIpc handle (any byte channel carries it: a file, a socket)
//   open_ipc     another PROCESS maps that allocation: a read-only handle with streams / workspaces of its own.  The caller passes
//                the owner's geometry (rows, columns, column capacity, hashes: bigsi_hip_get_info there).  The owner must stay
//                alive and must not close / re-stride (reserve_cols) the index while handles are attached.
//   open_view    another THREAD of the owner's process: the same, without the mapping (hipIpc does not open a handle in the
//                process that made it).  The owner handle must outlive its views.
static_assert(sizeof(hipIpcMemHandle_t) == BIGSI_IPC_HANDLE_BYTES, "hipIpc handle size");

extern "C" int bigsi_hip_export_ipc(bigsi_hip_index *ix, uint8_t *handle)
{
    if (!ix || !handle) return fail(BIGSI_ERR_INVALID, "NULL argument");
    BIGSI_ENTER(ix);
    if (ix->attach != bigsi_hip_index::kOwner) return fail(BIGSI_ERR_STATE, "only the handle that owns the matrix can export it");
    TRY(use_device(ix));
    TRY(quiesce_index(ix));
    HIP_TRY(hipStreamSynchronize(ix->stream));       // whatever filled the matrix is visible to the process that maps it next
    hipIpcMemHandle_t h;
    HIP_TRY(hipIpcGetMemHandle(&h, ix->d_index));
    memcpy(handle, &h, sizeof h);
    return BIGSI_OK;
}

extern "C" int bigsi_hip_open_ipc(const uint8_t *handle, uint64_t num_rows, uint64_t num_cols, uint64_t col_capacity, uint32_t num_hashes,
                                  int device, bigsi_hip_index **out)
{
    if (!handle) return fail(BIGSI_ERR_INVALID, "handle is NULL");
    if (num_cols > col_capacity) return fail(BIGSI_ERR_INVALID, "num_cols %llu exceeds the owner's column capacity %llu", (unsigned long long)num_cols, (unsigned long long)col_capacity);
    hipIpcMemHandle_t h;
    memcpy(&h, handle, sizeof h);
    return open_impl(num_rows, num_cols, col_capacity, num_hashes, device, &h, nullptr, out);
}

extern "C" int bigsi_hip_open_view(bigsi_hip_index *owner, bigsi_hip_index **out)
{
    if (!owner || !out) return fail(BIGSI_ERR_INVALID, "NULL argument");
    BIGSI_ENTER(owner);
    TRY(use_device(owner));
    TRY(quiesce_index(owner));
    HIP_TRY(hipStreamSynchronize(owner->stream));    // (streams of different handles are not ordered with each other)
    TRY(open_impl(owner->m, owner->n_cols, owner->cap_cols, owner->h, owner->device, nullptr, owner, out));
    return BIGSI_OK;
}

static void recycle_events(bigsi_hip_index *ix)
{
    for (auto *v : {&ix->ev_and, &ix->ev_km, &ix->ev_cp, &ix->ev_pr, &ix->ev_tr, &ix->ev_ex}) {
        for (auto &p : *v) ix->ev_free.push_back(p);
        v->clear();
    }
}

// A workspace of the index is given up: the slot first, then the batch (which waits for its work).  Leaves the thread's error message
// of a failed call in place.
static void drop_workspace(bigsi_hip_batch *&w)
{
    bigsi_hip_batch *b = w;
    w = nullptr;
    if (b) bigsi_hip_batch_destroy(b);
}

extern "C" int bigsi_hip_close(bigsi_hip_index *ix)
{
    if (!ix) return BIGSI_OK;
    {
        BusyGuard g(ix);
        if (!g.ok) return fail(BIGSI_ERR_STATE, "bigsi_hip_close: the handle is in use by another host thread");
        g.release();      // (the guard must not outlive the handle; whoever closes a handle owns it)
    }
    if (ix->views.load() > 0) return fail(BIGSI_ERR_STATE, "bigsi_hip_close: %d view(s) of this index are still open (close them first)", ix->views.load());
    const std::pair<bigsi_hip_batch **, int> workspaces[] = {{&ix->search_ws, 1},   {ix->stream_ws, 4},   {&ix->prevalence_ws, 1},
                                                             {ix->tally_ws, 2},     {ix->classify_ws, 2}, {&ix->window_ws, 1},
                                                             {ix->associate_ws, 2}, {ix->genotype_ws, 2}, {ix->typing_ws, 2}};
    for (const auto &[ws, n] : workspaces)
        for (int i = 0; i < n; i++) drop_workspace(ws[i]);
    hipError_t e = hipSetDevice(ix->device);
    e = hipStreamSynchronize(ix->stream);
    if (ix->pre_stream) e = hipStreamSynchronize(ix->pre_stream);
    for (auto st : ix->rd_stream)
        if (st) { e = hipStreamSynchronize(st); e = hipStreamDestroy(st); }
    if (ix->sc_stream) { e = hipStreamSynchronize(ix->sc_stream); e = hipStreamDestroy(ix->sc_stream); }
    if (ix->main_ev) e = hipEventDestroy(ix->main_ev);
    recycle_events(ix);
    for (auto &p : ix->ev_free) { e = hipEventDestroy(p.a); e = hipEventDestroy(p.b); }
    ix->stage.release();
    ix->stage_ids.release();
    for (int s_ = 0; s_ < 2; s_++) {
        if (ix->pin_rows[s_]) e = hipHostFree(ix->pin_rows[s_]);
        if (ix->pin_ev[s_]) e = hipEventDestroy(ix->pin_ev[s_]);
        ix->dev_rows[s_].release();
        ix->dev_ids[s_].release();
        if (ix->classify_pin[s_]) e = hipHostFree(ix->classify_pin[s_]);
        if (ix->classify_ev[s_]) e = hipEventDestroy(ix->classify_ev[s_]);
        ix->classify_rec[s_].release();
        if (ix->associate_pin[s_]) e = hipHostFree(ix->associate_pin[s_]);
        if (ix->associate_ev[s_]) e = hipEventDestroy(ix->associate_ev[s_]);
        ix->associate_out[s_].release();
    }
    ix->classify_groups.release();
    ix->associate_groups.release();
    ix->associate_masks.release();
    if (ix->view_of) ix->view_of->views--;
    if (ix->d_index && ix->attach == bigsi_hip_index::kOwner) e = hipFree(ix->d_index);
    else if (ix->d_index && ix->attach == bigsi_hip_index::kIpc) e = hipIpcCloseMemHandle(ix->d_index);
    if (ix->own_stream) e = hipStreamDestroy(ix->own_stream);
    if (ix->pre_stream) e = hipStreamDestroy(ix->pre_stream);
    (void)e;
    delete ix;
    return BIGSI_OK;
}

extern "C" int bigsi_hip_get_info(const bigsi_hip_index *ix, bigsi_hip_info *out)
{
    if (!ix || !out) return fail(BIGSI_ERR_INVALID, "NULL argument");
    out->num_rows = ix->m;
    out->num_cols = ix->n_cols;
    out->col_capacity = ix->cap_cols;
    out->row_bytes = ix->rb();
    out->row_stride_bytes = ix->stride_words * 8;
    out->index_bytes = ix->m * ix->stride_words * 8;
    out->num_hashes = ix->h;
    out->device = ix->device;
    return BIGSI_OK;
}

extern "C" int bigsi_hip_set_num_cols(bigsi_hip_index *ix, uint64_t num_cols)
{
    BIGSI_ENTER(ix);
    if (!ix) return fail(BIGSI_ERR_INVALID, "NULL index");
    if (num_cols > ix->cap_cols)
        return fail(BIGSI_ERR_CAPACITY, "num_cols %llu exceeds col_capacity %llu (call bigsi_hip_reserve_cols)",
                    (unsigned long long)num_cols, (unsigned long long)ix->cap_cols);
    ix->n_cols = num_cols;
    return BIGSI_OK;
}

extern "C" int bigsi_hip_set_num_hashes(bigsi_hip_index *ix, uint32_t num_hashes)
{
    BIGSI_ENTER(ix);
    if (!ix) return fail(BIGSI_ERR_INVALID, "NULL index");
    if (num_hashes == 0) return fail(BIGSI_ERR_INVALID, "num_hashes must be > 0");
    ix->h = num_hashes;
    return BIGSI_OK;
}

extern "C" int bigsi_hip_reserve_cols(bigsi_hip_index *ix, uint64_t col_capacity)
{
    BIGSI_ENTER(ix);
    if (!ix) return fail(BIGSI_ERR_INVALID, "NULL index");
    if (col_capacity <= ix->cap_cols) return BIGSI_OK;          // (only a call that would really re-stride the matrix needs to own it)
    if (col_capacity > 0xFFFFFFFFull) return fail(BIGSI_ERR_INVALID, "col_capacity exceeds 2^32-1");
    TRY(begin_rewrite(ix, "bigsi_hip_reserve_cols", "re-striding would move the matrix under them"));
    return replace_matrix(ix, stride_for(col_capacity), "bigsi_hip_reserve_cols");
}

extern "C" int bigsi_hip_set_stream(bigsi_hip_index *ix, void *hip_stream)
{
    BIGSI_ENTER(ix);
    if (!ix) return fail(BIGSI_ERR_INVALID, "NULL index");
    TRY(use_device(ix));
    TRY(quiesce_index(ix));
    HIP_TRY(hipStreamSynchronize(ix->stream));
    ix->stream = hip_stream ? (hipStream_t)hip_stream : ix->own_stream;
    return BIGSI_OK;
}

extern "C" int bigsi_hip_synchronize(bigsi_hip_index *ix)
{
    BIGSI_ENTER(ix);
    if (!ix) return fail(BIGSI_ERR_INVALID, "NULL index");
    TRY(use_device(ix));
    TRY(quiesce_index(ix));
    HIP_TRY(hipStreamSynchronize(ix->pre_stream));
    HIP_TRY(hipStreamSynchronize(ix->stream));
    return BIGSI_OK;
}

// ------------------------------------------------------------------------------ storage contract
static const uint64_t kStageBytes = 64ull << 20;
static const uint64_t kZeroCopyBytes = 256ull << 10;     // inputs of a one-call search up to this size are read by K1 from pinned memory

extern "C" int bigsi_hip_set_rows(bigsi_hip_index *ix, const uint64_t *row_ids, uint64_t n, const uint8_t *bytes, uint64_t row_bytes)
{
    BIGSI_ENTER(ix);
    TRY(bigsi_writable(ix));
    if (!ix || (n && (!row_ids || !bytes))) return fail(BIGSI_ERR_INVALID, "NULL argument");
    if (row_bytes == 0 || row_bytes > ix->stride_words * 8)
        return fail(BIGSI_ERR_CAPACITY, "row_bytes %llu not in [1, %llu] (row stride)", (unsigned long long)row_bytes,
                    (unsigned long long)(ix->stride_words * 8));
    for (uint64_t i = 0; i < n; i++)
        if (row_ids[i] >= ix->m) return fail(BIGSI_ERR_RANGE, "row %llu out of range [0,%llu)", (unsigned long long)row_ids[i], (unsigned long long)ix->m);
    TRY(use_device(ix));
    TRY(quiesce_index(ix));
    const uint64_t kMaxChunkRows = 1ull << 20;      // (the pinned buffers keep room for this many row ids behind the row bytes)
    const uint64_t per = std::min(kMaxChunkRows, std::max<uint64_t>(1, kStageBytes / row_bytes));
    if (n * row_bytes < (4ull << 20) || row_bytes > kStageBytes) {
        // a few rows (the storage contract's own calls): one staged copy.  Rows wider than a pinned buffer of the route below (64 MB:
        // more than 512 M columns) come this way too, one row at a time -- that route sizes its buffers for kStageBytes and would
        // overrun them (round-5 advisor)
        const uint64_t rows_at_once = row_bytes > kStageBytes ? 1 : n;
        for (uint64_t i0 = 0; i0 < n; i0 += rows_at_once) {
            const uint64_t c = std::min(rows_at_once, n - i0);
            TRY(ix->stage.reserve(c * row_bytes));
            TRY(ix->stage_ids.reserve(c * 8));
            HIP_TRY(hipMemcpyAsync(ix->stage.p, bytes + i0 * row_bytes, c * row_bytes, hipMemcpyHostToDevice, ix->stream));
            HIP_TRY(hipMemcpyAsync(ix->stage_ids.p, row_ids + i0, c * 8, hipMemcpyHostToDevice, ix->stream));
            hipLaunchKernelGGL(k_scatter_rows, dim3((unsigned)c), dim3(kBlock), 0, ix->stream, (uint8_t *)ix->d_index,
                               ix->stride_words * 8, ix->m, ix->stage_ids.as<uint64_t>(), ix->stage.as<uint8_t>(), row_bytes);
            HIP_TRY(hipGetLastError());
            HIP_TRY(hipStreamSynchronize(ix->stream));
        }
        return BIGSI_OK;
    }
    // blocks of rows (importers: migrate_index, bdb.import_index): the caller's pageable memory goes into one of two pinned
    // buffers on a few host threads while the other buffer's copy and scatter kernel are in flight (a hipMemcpy from pageable
    // memory stages through the runtime's own small buffers on one thread: 7-8 GB/s)
    for (int s_ = 0; s_ < 2; s_++) {
        if (!ix->pin_rows[s_]) HIP_TRY(hipHostMalloc(&ix->pin_rows[s_], kStageBytes + kMaxChunkRows * 8, hipHostMallocDefault));
        if (!ix->pin_ev[s_]) HIP_TRY(hipEventCreateWithFlags(&ix->pin_ev[s_], hipEventDisableTiming));
        TRY(ix->dev_rows[s_].reserve(kStageBytes));
        TRY(ix->dev_ids[s_].reserve(per * 8));
    }
    const unsigned T = std::min(8u, std::max(1u, std::thread::hardware_concurrency() / 8));
    uint64_t chunk = 0;
    for (uint64_t i0 = 0; i0 < n; i0 += per, chunk++) {
        const int s_ = (int)(chunk & 1);
        const uint64_t c = std::min(per, n - i0), nb = c * row_bytes;
        HIP_TRY(hipEventSynchronize(ix->pin_ev[s_]));          // (never recorded: returns at once) the copy that last read this buffer
        uint8_t *pin = static_cast<uint8_t *>(ix->pin_rows[s_]);
        const uint8_t *src = bytes + i0 * row_bytes;
        {
            std::vector<std::thread> pool;
            const uint64_t part = round_up(ceil_div(nb, T), 1 << 16);
            for (unsigned t = 1; t < T; t++) {
                const uint64_t a = std::min<uint64_t>((uint64_t)t * part, nb), b = std::min<uint64_t>((uint64_t)(t + 1) * part, nb);
                if (a < b) pool.emplace_back([=]() { memcpy(pin + a, src + a, b - a); });
            }
            memcpy(pin, src, std::min(part, nb));
            for (auto &th : pool) th.join();
        }
        memcpy(pin + kStageBytes, row_ids + i0, c * 8);
        HIP_TRY(hipMemcpyAsync(ix->dev_rows[s_].p, pin, nb, hipMemcpyHostToDevice, ix->stream));
        HIP_TRY(hipMemcpyAsync(ix->dev_ids[s_].p, pin + kStageBytes, c * 8, hipMemcpyHostToDevice, ix->stream));
        hipLaunchKernelGGL(k_scatter_rows, dim3((unsigned)c), dim3(kBlock), 0, ix->stream, (uint8_t *)ix->d_index,
                           ix->stride_words * 8, ix->m, ix->dev_ids[s_].as<uint64_t>(), ix->dev_rows[s_].as<uint8_t>(), row_bytes);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipEventRecord(ix->pin_ev[s_], ix->stream));
    }
    HIP_TRY(hipStreamSynchronize(ix->stream));
    return BIGSI_OK;
}

extern "C" int bigsi_hip_get_rows(bigsi_hip_index *ix, const uint64_t *row_ids, uint64_t n, uint8_t *out, uint64_t row_bytes)
{
    BIGSI_ENTER(ix);
    if (!ix || (n && (!row_ids || !out))) return fail(BIGSI_ERR_INVALID, "NULL argument");
    if (row_bytes == 0) return fail(BIGSI_ERR_INVALID, "row_bytes is 0");
    for (uint64_t i = 0; i < n; i++)
        if (row_ids[i] >= ix->m) return fail(BIGSI_ERR_RANGE, "row %llu out of range [0,%llu)", (unsigned long long)row_ids[i], (unsigned long long)ix->m);
    TRY(use_device(ix));
    const uint64_t per = std::max<uint64_t>(1, kStageBytes / row_bytes);
    for (uint64_t i0 = 0; i0 < n; i0 += per) {
        const uint64_t c = std::min(per, n - i0);
        TRY(ix->stage.reserve(c * row_bytes));
        TRY(ix->stage_ids.reserve(c * 8));
        HIP_TRY(hipMemcpyAsync(ix->stage_ids.p, row_ids + i0, c * 8, hipMemcpyHostToDevice, ix->stream));
        hipLaunchKernelGGL(k_gather_rows, dim3((unsigned)c), dim3(kBlock), 0, ix->stream, (const uint8_t *)ix->d_index,
                           ix->stride_words * 8, ix->m, ix->stage_ids.as<uint64_t>(), ix->stage.as<uint8_t>(), row_bytes);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(out + i0 * row_bytes, ix->stage.p, c * row_bytes, hipMemcpyDeviceToHost, ix->stream));
        HIP_TRY(hipStreamSynchronize(ix->stream));
    }
    return BIGSI_OK;
}

// ------------------------------------------------------------------------------ bulk ingest: file <-> HBM
// The reference loads an index by opening a BerkeleyDB file (bigsi/storage/berkeleydb.py:6-19) and pays a page lookup + two copies
// per row at query time; here the rows go to HBM once, at the rate the file system and PCIe allow: the file range is read by
// `threads` host threads (pread, one slice each) into one of two pinned buffers while the other one is in flight to the device
// (hipMemcpyAsync; rows whose file length is not the device pitch take one scatter kernel on the way).  File side: bigsi_rowsfile.cpp.
int bigsi_rows_pipeline(const BigsiRowsDevice &dev, unsigned pin_flags, const char *path, uint64_t file_offset, uint64_t row0, uint64_t n_rows,
                        uint64_t row_bytes, uint32_t threads, bool save, bool direct, bigsi_hip_io_stats *st)
{
    BigsiRowsFile rf;
    TRY(rf.open_(path, save, file_offset, row_bytes, n_rows, row0, threads));
    const uint64_t per = rf.chunk_rows();
    uint8_t *pin[2] = {nullptr, nullptr};
    const auto t_begin = std::chrono::steady_clock::now();
    double io_s = 0;
    auto file_io = [&](int slot, uint64_t c) -> int {                   // chunk c between pin[slot] and the file
        const auto t0 = std::chrono::steady_clock::now();
        const int e = rf.io(save, pin[slot], c * per, std::min(per, n_rows - c * per), threads);
        io_s += std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
        if (e && save) return fail(BIGSI_ERR_INVALID, "writing %s: %s", path, strerror(e));
        if (e) return fail(BIGSI_ERR_INVALID, "reading %s: %s", path, e == ENODATA ? "file too short" : strerror(e));
        return BIGSI_OK;
    };
    auto copies = [&](int slot, uint64_t c) { return dev.queue(slot, pin[slot], row0 + c * per, std::min(per, n_rows - c * per)); };      // ... and the device(s)
    auto body = [&]() -> int {
        const uint64_t buf_bytes = std::min(per, std::max<uint64_t>(n_rows, 1)) * row_bytes;
        for (auto &p : pin) HIP_TRY(hipHostMalloc(reinterpret_cast<void **>(&p), buf_bytes, pin_flags));
        TRY(dev.prepare(buf_bytes));
        const uint64_t n_chunks = ceil_div(n_rows, per);
        // load:  read(c) | copies(c) in flight while read(c + 1) runs;   save:  copies(c + 1) in flight while write(c) runs
        for (uint64_t c = 0; c < n_chunks + (save ? 1 : 0); c++) {
            const int slot = (int)(c & 1);
            if (save) {
                if (c < n_chunks) TRY(copies(slot, c));                  // queued, not waited for
                if (c > 0) {                                             // write chunk c - 1 while chunk c comes down
                    TRY(dev.wait(slot ^ 1));
                    TRY(file_io(slot ^ 1, c - 1));
                }
            } else {
                TRY(dev.wait(slot));                                     // (never recorded: returns at once) the copies that last read this buffer
                TRY(file_io(slot, c));
                TRY(copies(slot, c));
            }
        }
        for (int s = 0; s < 2; s++) TRY(dev.wait(s));
        return BIGSI_OK;
    };
    int rc = body();
    if (save && rc == BIGSI_OK) { const int e_ = rf.sync_all(); if (e_) rc = fail(BIGSI_ERR_INVALID, "fsync %s: %s", path, strerror(e_)); }
    char keep[1024] = "";
    if (rc != BIGSI_OK) snprintf(keep, sizeof keep, "%s", bigsi_hip_last_error());      // (the clean-up below must not overwrite the message)
    dev.release();                                                       // drains every stream first: nothing reads a buffer that is freed
    for (auto p : pin)
        if (p) { hipError_t e = hipHostFree(p); (void)e; }
    rf.close_();
    if (rc != BIGSI_OK) return fail(rc, "%s", keep);
    if (st) {
        st->bytes = n_rows * row_bytes;
        st->seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t_begin).count();
        st->file_seconds = io_s;
        st->threads = threads;
        st->direct = direct ? 1u : 0u;
    }
    return BIGSI_OK;
}

namespace {
int rows_file(bigsi_hip_index *ix, const char *path, uint64_t file_offset, uint64_t row0, uint64_t n_rows, uint64_t row_bytes, uint32_t threads,
              bool save, bigsi_hip_io_stats *st)
{
    if (!ix || !path) return fail(BIGSI_ERR_INVALID, "NULL argument");
    const uint64_t stride = ix->stride_words * 8;
    if (row_bytes == 0 || (!save && row_bytes > stride))
        return fail(BIGSI_ERR_CAPACITY, "row_bytes %llu not in [1, %llu] (row stride)", (unsigned long long)row_bytes, (unsigned long long)stride);
    if (row0 > ix->m || n_rows > ix->m - row0) return fail(BIGSI_ERR_RANGE, "rows [%llu, +%llu) outside [0, %llu)", (unsigned long long)row0, (unsigned long long)n_rows, (unsigned long long)ix->m);
    if (threads == 0) threads = bigsi_io_threads();
    TRY(use_device(ix));
    TRY(quiesce_index(ix));
    HIP_TRY(hipStreamSynchronize(ix->stream));
    const bool direct = row_bytes == stride;                         // the file holds the device layout: no kernel on the way
    uint8_t *base = reinterpret_cast<uint8_t *>(ix->d_index);
    hipEvent_t ev[2] = {nullptr, nullptr};
    DevBuf dev[2];                                                 // not direct: a chunk at the file's pitch, between the copy and the kernel
    BigsiRowsDevice side;
    side.prepare = [&](uint64_t buf_bytes) -> int {
        for (int i = 0; i < 2; i++) {
            HIP_TRY(hipEventCreateWithFlags(&ev[i], hipEventDisableTiming));
            if (!direct) TRY(dev[i].reserve(buf_bytes));
        }
        return BIGSI_OK;
    };
    side.queue = [&](int slot, uint8_t *pin, uint64_t r0, uint64_t cn) -> int {
        if (save) {
            if (direct) HIP_TRY(hipMemcpyAsync(pin, base + r0 * stride, cn * row_bytes, hipMemcpyDeviceToHost, ix->stream));
            else {
                hipLaunchKernelGGL(k_gather_run, dim3((unsigned)cn), dim3(kBlock), 0, ix->stream, base, stride, r0, dev[slot].as<uint8_t>(), row_bytes);
                HIP_TRY(hipGetLastError());
                HIP_TRY(hipMemcpyAsync(pin, dev[slot].p, cn * row_bytes, hipMemcpyDeviceToHost, ix->stream));
            }
        } else {
            if (direct) HIP_TRY(hipMemcpyAsync(base + r0 * stride, pin, cn * row_bytes, hipMemcpyHostToDevice, ix->stream));
            else {
                HIP_TRY(hipMemcpyAsync(dev[slot].p, pin, cn * row_bytes, hipMemcpyHostToDevice, ix->stream));
                hipLaunchKernelGGL(k_scatter_run, dim3((unsigned)cn), dim3(kBlock), 0, ix->stream, base, stride, r0, dev[slot].as<uint8_t>(), row_bytes);
                HIP_TRY(hipGetLastError());
            }
        }
        HIP_TRY(hipEventRecord(ev[slot], ix->stream));
        return BIGSI_OK;
    };
    side.wait = [&](int slot) -> int {
        HIP_TRY(hipEventSynchronize(ev[slot]));
        return BIGSI_OK;
    };
    side.release = [&]() {
        hipError_t e = hipStreamSynchronize(ix->stream);
        for (int i = 0; i < 2; i++) {
            if (ev[i]) e = hipEventDestroy(ev[i]);
            dev[i].release();
        }
        (void)e;
    };
    return bigsi_rows_pipeline(side, hipHostMallocDefault, path, file_offset, row0, n_rows, row_bytes, threads, save, direct, st);
}
}   // namespace

extern "C" int bigsi_hip_load_rows_file(bigsi_hip_index *ix, const char *path, uint64_t file_offset, uint64_t row0, uint64_t n_rows, uint64_t row_bytes,
                                        uint32_t threads, bigsi_hip_io_stats *stats)
{
    BIGSI_ENTER(ix);
    TRY(bigsi_writable(ix));
    return rows_file(ix, path, file_offset, row0, n_rows, row_bytes, threads, false, stats);
}

extern "C" int bigsi_hip_save_rows_file(bigsi_hip_index *ix, const char *path, uint64_t file_offset, uint64_t row0, uint64_t n_rows, uint64_t row_bytes,
                                        uint32_t threads, bigsi_hip_io_stats *stats)
{
    BIGSI_ENTER(ix);
    return rows_file(ix, path, file_offset, row0, n_rows, row_bytes, threads, true, stats);
}

extern "C" int bigsi_hip_clear(bigsi_hip_index *ix)
{
    BIGSI_ENTER(ix);
    TRY(bigsi_writable(ix));
    if (!ix) return fail(BIGSI_ERR_INVALID, "NULL index");
    TRY(use_device(ix));
    TRY(quiesce_index(ix));
    HIP_TRY(hipMemsetAsync(ix->d_index, 0, (size_t)ix->m * ix->stride_words * 8, ix->stream));
    HIP_TRY(hipStreamSynchronize(ix->stream));
    return BIGSI_OK;
}

extern "C" int bigsi_hip_insert_column(bigsi_hip_index *ix, uint64_t col, const uint8_t *bloom)
{
    BIGSI_ENTER(ix);
    TRY(bigsi_writable(ix));
    if (!ix || !bloom) return fail(BIGSI_ERR_INVALID, "NULL argument");
    if (col > ix->n_cols) return fail(BIGSI_ERR_RANGE, "column %llu beyond num_cols %llu", (unsigned long long)col, (unsigned long long)ix->n_cols);
    if (col >= ix->cap_cols) return fail(BIGSI_ERR_CAPACITY, "column %llu beyond col_capacity %llu", (unsigned long long)col, (unsigned long long)ix->cap_cols);
    TRY(use_device(ix));
    TRY(quiesce_index(ix));
    const uint64_t nb = ceil_div(ix->m, 8);
    TRY(ix->stage.reserve(nb));
    HIP_TRY(hipMemcpyAsync(ix->stage.p, bloom, nb, hipMemcpyHostToDevice, ix->stream));
    const unsigned grid = (unsigned)std::min<uint64_t>(ceil_div(ix->m, kBlock), 256 * 8);
    hipLaunchKernelGGL(k_insert_column, dim3(grid), dim3(kBlock), 0, ix->stream, ix->d_index, ix->stride_words, ix->m, col, ix->stage.as<uint8_t>());
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(ix->stream));
    if (col == ix->n_cols) ix->n_cols++;
    return BIGSI_OK;
}

#define ev_begin bigsi_ev_begin
#define ev_end bigsi_ev_end

// n filters already on the device -> columns [col0, col0 + n): whole 64-column words through the tiled transpose
// (k_transpose_regs), the ragged head (up to the next multiple of 128 columns) and tail through k_insert_columns
static int transpose_device(bigsi_hip_index *ix, uint64_t col0, uint64_t n, const uint8_t *d_blooms, uint64_t bstride)
{
    const uint64_t nb = ceil_div(ix->m, 8), end = col0 + n;
    auto slow = [&](uint64_t ca, uint64_t cnt) -> int {
        if (!cnt) return BIGSI_OK;
        const uint64_t items = ix->m * (((ca + cnt - 1) >> 6) - (ca >> 6) + 1);
        const unsigned grid = (unsigned)std::min<uint64_t>(ceil_div(items, kBlock), 256 * 32);
        hipLaunchKernelGGL(k_insert_columns, dim3(grid), dim3(kBlock), 0, ix->stream, ix->d_index, ix->stride_words, ix->m, ca, cnt,
                           d_blooms + (ca - col0) * bstride, bstride);
        HIP_TRY(hipGetLastError());
        return BIGSI_OK;
    };
    const uint64_t c_lo = std::min(end, round_up(col0, 128));
    uint64_t n_words = (end - c_lo) / 64, c_hi = c_lo + n_words * 64;
    // XCD groups of 4 rows x 1 column of supertiles (A/B in profiles/r06_transpose_regs_ab.txt)
    constexpr uint32_t tr_rg = 4, tr_cg = 1;
    // k_transpose_regs<2>: 1024 rows x 1024 columns per workgroup -- whole 128-byte lines of the filters in (two consecutive loads per
    // lane), 128-byte runs of the rows out.  (RT = 1, 512 rows: 4.4-5.0 TB/s against 4.9-5.4, its half lines shared with another workgroup.)
    constexpr uint64_t rt = 2, ct = 2;
    // APPENDING (nothing valid at or beyond `end`: the usual build) the tiled kernel also takes the ragged tail: it writes whole 128-byte
    // lines, zeros for the columns that have no filter -- what those bits of the row hold anyway -- instead of leaving up to 63 columns to
    // the column-at-a-time kernel and a partly written line to the memory (round 6: 1 M x 100 000 against 1 M x 98 304: -5 %)
    if (end >= ix->n_cols && end > c_lo) {
        n_words = std::min<uint64_t>(round_up(ceil_div(end - c_lo, 64), 16), ix->stride_words - c_lo / 64);
        c_hi = end;
    }
    // supertiles of 1024 tiles: 32 wide, narrower (and higher) when the matrix has fewer tile columns than that
    const uint64_t tiles_c = ceil_div(n_words, 8 * ct);
    uint32_t sup_w = kTransposeSuper;
    while (sup_w > 1 && sup_w / 2 >= tiles_c) sup_w /= 2;
    const uint32_t sup_h = (uint32_t)(kTransposeSuper * kTransposeSuper) / sup_w;
    const uint64_t sup_blocks = ceil_div(ceil_div(ix->m, kTransposeTile * rt), sup_h) * ceil_div(tiles_c, sup_w) * (uint64_t)(kTransposeSuper * kTransposeSuper);
    if (n_words == 0 || bstride % 16 || ((uintptr_t)d_blooms & 15u) || sup_blocks > 0x7FFFFFFFull) return slow(col0, n);
    TRY(slow(col0, c_lo - col0));
    hipLaunchKernelGGL(k_transpose_regs<2>, dim3((unsigned)sup_blocks), dim3(kBlock * (unsigned)ct), 0, ix->stream, ix->d_index, ix->stride_words,
                       ix->m, c_lo / 64, n_words, d_blooms + (c_lo - col0) * bstride, end - c_lo, bstride, nb, tr_rg, tr_cg, sup_w);
    HIP_TRY(hipGetLastError());
    return slow(c_hi, end - c_hi);
}

static int check_insert_columns(bigsi_hip_index *ix, uint64_t col0, uint64_t n, const void *blooms, uint64_t bloom_stride_bytes)
{
    if (!ix || (n && !blooms)) return fail(BIGSI_ERR_INVALID, "NULL argument");
    const uint64_t nb = ceil_div(ix->m, 8);
    if (n && bloom_stride_bytes < nb) return fail(BIGSI_ERR_INVALID, "bloom_stride_bytes %llu < ceil(num_rows/8) = %llu", (unsigned long long)bloom_stride_bytes, (unsigned long long)nb);
    if (col0 > ix->n_cols) return fail(BIGSI_ERR_RANGE, "column %llu beyond num_cols %llu", (unsigned long long)col0, (unsigned long long)ix->n_cols);
    if (col0 + n > ix->cap_cols) return fail(BIGSI_ERR_CAPACITY, "columns [%llu,%llu) beyond col_capacity %llu", (unsigned long long)col0, (unsigned long long)(col0 + n), (unsigned long long)ix->cap_cols);
    return BIGSI_OK;
}

extern "C" int bigsi_hip_insert_columns(bigsi_hip_index *ix, uint64_t col0, uint64_t n, const uint8_t *blooms, uint64_t bloom_stride_bytes)
{
    BIGSI_ENTER(ix);
    TRY(bigsi_writable(ix));
    TRY(check_insert_columns(ix, col0, n, blooms, bloom_stride_bytes));
    if (n == 0) return BIGSI_OK;
    TRY(use_device(ix));
    TRY(quiesce_index(ix));
    // filters are staged a slab at a time at a 128-byte pitch -- the transpose reads a filter in 128-byte runs, and a run that
    // straddles two L2 lines is fetched twice by neighbouring tiles (round 6, TCC_EA0_RDREQ_128B: 1.32 x the filter bytes at a
    // 16-byte pitch, 1.0 x at this one) --: at least 512 of them when 2 GB allow it (one transpose tile is 512 columns wide),
    // otherwise about 256 MB worth
    // (a pitch that is a multiple of 4 KB puts the same line of all the filters of a tile on few memory channels: 2 M-row filters at a
    //  256 KB pitch transpose at 4.5-4.8 TB/s against 5.0-5.3 one line further apart)
    const uint64_t nb = ceil_div(ix->m, 8), pitch = round_up(nb, 128) + (round_up(nb, 128) % 4096 == 0 ? 128 : 0);
    const uint64_t stage_bytes = std::min<uint64_t>(std::max<uint64_t>(512 * pitch, 256ull << 20), 2048ull << 20);
    uint64_t per = std::max<uint64_t>(1, stage_bytes / pitch);
    if (per >= 128) per = per / 128 * 128;
    for (uint64_t c0 = 0; c0 < n; c0 += per) {
        const uint64_t cn = std::min(per, n - c0);
        TRY(ix->stage.reserve(cn * pitch));
        HIP_TRY(hipMemcpy2DAsync(ix->stage.p, pitch, blooms + c0 * bloom_stride_bytes, bloom_stride_bytes, nb, cn, hipMemcpyHostToDevice, ix->stream));
        TRY(transpose_device(ix, col0 + c0, cn, ix->stage.as<uint8_t>(), pitch));
        HIP_TRY(hipStreamSynchronize(ix->stream));
    }
    if (col0 + n > ix->n_cols) ix->n_cols = col0 + n;
    return BIGSI_OK;
}

extern "C" int bigsi_hip_insert_columns_device(bigsi_hip_index *ix, uint64_t col0, uint64_t n, const void *d_blooms, uint64_t bloom_stride_bytes)
{
    BIGSI_ENTER(ix);
    TRY(bigsi_writable(ix));
    TRY(check_insert_columns(ix, col0, n, d_blooms, bloom_stride_bytes));
    if (n == 0) return BIGSI_OK;
    TRY(use_device(ix));
    TRY(quiesce_index(ix));
    EventPair ep{};
    TRY(ev_begin(ix, &ep));
    TRY(transpose_device(ix, col0, n, (const uint8_t *)d_blooms, bloom_stride_bytes));
    TRY(ev_end(ix, &ep, ix->ev_tr));
    HIP_TRY(hipStreamSynchronize(ix->stream));
    if (col0 + n > ix->n_cols) ix->n_cols = col0 + n;
    return BIGSI_OK;
}

extern "C" int bigsi_hip_append_index(bigsi_hip_index *dst, const bigsi_hip_index *src)
{
    BIGSI_ENTER_DERIVE(dst, src);
    TRY(check_derive({"bigsi_hip_append_index", /*in_place*/ nullptr, /*rows_divide*/ false, /*same_hashes*/ false, /*into_empty*/ false}, dst, src));
    if (src->n_cols == 0) return BIGSI_OK;
    TRY(begin_derive(dst, src, dst->n_cols + src->n_cols));
    const uint64_t per_row = ceil_div(dst->n_cols + src->n_cols, 64) - (dst->n_cols >> 6);
    const unsigned grid = (unsigned)std::min<uint64_t>(ceil_div(dst->m * per_row, kBlock), 256 * 64);
    hipLaunchKernelGGL(k_append_columns, dim3(grid), dim3(kBlock), 0, dst->stream, dst->d_index, dst->stride_words, dst->n_cols,
                       src->d_index, src->stride_words, src->n_cols, dst->m);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(dst->stream));
    dst->n_cols += src->n_cols;
    return BIGSI_OK;
}

extern "C" int bigsi_hip_get_column(bigsi_hip_index *ix, uint64_t col, uint8_t *out)
{
    BIGSI_ENTER(ix);
    if (!ix || !out) return fail(BIGSI_ERR_INVALID, "NULL argument");
    // (a column the index does not have is refused, as the CPU twin refuses it: what the stride holds behind num_cols is no sample's filter)
    if (col >= ix->n_cols) return fail(BIGSI_ERR_RANGE, "column %llu out of range [0,%llu)", (unsigned long long)col, (unsigned long long)ix->n_cols);
    TRY(use_device(ix));
    const uint64_t nb = ceil_div(ix->m, 8);
    TRY(ix->stage.reserve(nb));
    const unsigned grid = (unsigned)std::min<uint64_t>(ceil_div(nb, kBlock), 256 * 8);
    hipLaunchKernelGGL(k_get_column, dim3(grid), dim3(kBlock), 0, ix->stream, ix->d_index, ix->stride_words, ix->m, col, ix->stage.as<uint8_t>());
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(out, ix->stage.p, nb, hipMemcpyDeviceToHost, ix->stream));
    HIP_TRY(hipStreamSynchronize(ix->stream));
    return BIGSI_OK;
}

// Sample statistics: the vertical popcount (k_col_popcount, launch shape: plan_col_popcount).  The partial counters of the row blocks
// live for this call only (a few MB for a test index, ~130 MB beside a 125 GB one): statistics are asked for now and then, not in a
// serving loop, so the handle keeps nothing resident for them.
namespace {
struct CallScratch {
    DevBuf buf;
    ~CallScratch() { buf.release(); }
};
}  // namespace

extern "C" int bigsi_hip_column_popcounts(bigsi_hip_index *ix, const uint8_t *row_mask, uint64_t *out, uint64_t capacity)
{
    BIGSI_ENTER(ix);
    if (!ix || !out) return fail(BIGSI_ERR_INVALID, "NULL argument");
    if (capacity < ix->n_cols)
        return fail(BIGSI_ERR_CAPACITY, "capacity %llu is below num_cols %llu", (unsigned long long)capacity, (unsigned long long)ix->n_cols);
    if (ix->n_cols == 0) return BIGSI_OK;
    if (ix->m == 0) { memset(out, 0, ix->n_cols * 8); return BIGSI_OK; }
    TRY(use_device(ix));
    const ColPopPlan p = plan_col_popcount(ix->m, ix->stride_words);
    if (p.grid > 0x7FFFFFFFull) return fail(BIGSI_ERR_INVALID, "index too large for one popcount launch (%llu workgroups)", (unsigned long long)p.grid);
    CallScratch partial;
    TRY(partial.buf.reserve(p.row_blocks * p.partial_stride * 4));
    TRY(ix->stage_ids.reserve(ix->n_cols * 8));
    const uint64_t *d_mask = nullptr;
    if (row_mask) {
        const uint64_t words = ceil_div(ix->m, 64);
        TRY(ix->stage.reserve(words * 8));
        HIP_TRY(hipMemsetAsync(ix->stage.as<uint64_t>() + (words - 1), 0, 8, ix->stream));       // the bytes past ceil(m / 8) of the last word
        HIP_TRY(hipMemcpyAsync(ix->stage.p, row_mask, ceil_div(ix->m, 8), hipMemcpyHostToDevice, ix->stream));
        d_mask = ix->stage.as<uint64_t>();
    }
    if (d_mask)
        hipLaunchKernelGGL(k_col_popcount<true>, dim3((unsigned)p.grid), dim3(p.block), 0, ix->stream, ix->d_index, ix->stride_words, ix->m,
                           p.rows_per_block, (uint32_t)p.seg_groups, p.flush_groups, d_mask, partial.buf.as<uint32_t>(), p.partial_stride);
    else
        hipLaunchKernelGGL(k_col_popcount<false>, dim3((unsigned)p.grid), dim3(p.block), 0, ix->stream, ix->d_index, ix->stride_words, ix->m,
                           p.rows_per_block, (uint32_t)p.seg_groups, p.flush_groups, d_mask, partial.buf.as<uint32_t>(), p.partial_stride);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(k_col_popcount_sum, dim3((unsigned)ceil_div(ix->n_cols, kBlock)), dim3(kBlock), 0, ix->stream, partial.buf.as<uint32_t>(),
                       p.partial_stride, p.row_blocks, ix->n_cols, ix->stage_ids.as<uint64_t>());
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(out, ix->stage_ids.p, ix->n_cols * 8, hipMemcpyDeviceToHost, ix->stream));
    HIP_TRY(hipStreamSynchronize(ix->stream));
    return BIGSI_OK;
}

// Column compaction (k_compact_columns; tables and launch shape: plan_compact_columns).  The tables live for this call only, like the
// statistics' counters: 64 bytes per source word, 100 KB for 100 k columns.  `dst` may be `src` (in place: see the kernel).
static int compact_launch(bigsi_hip_index *dst, const bigsi_hip_index *src, const CompactPlan &p)
{
    if (p.kept == 0) {
        HIP_TRY(hipMemsetAsync(dst->d_index, 0, (size_t)dst->m * dst->stride_words * 8, dst->stream));
        HIP_TRY(hipStreamSynchronize(dst->stream));
        return BIGSI_OK;
    }
    CallScratch tab;
    const uint64_t words_bytes = p.src_words * sizeof(CompactWord), first_bytes = (p.dst_words + 1) * 4;
    TRY(tab.buf.reserve(words_bytes + first_bytes));
    HIP_TRY(hipMemcpyAsync(tab.buf.p, p.words.data(), words_bytes, hipMemcpyHostToDevice, dst->stream));
    HIP_TRY(hipMemcpyAsync(tab.buf.as<uint8_t>() + words_bytes, p.first_src.data(), first_bytes, hipMemcpyHostToDevice, dst->stream));
    hipLaunchKernelGGL(k_compact_columns, dim3((unsigned)p.grid), dim3(p.block), 0, dst->stream, src->d_index, src->stride_words, dst->d_index,
                       dst->stride_words, dst->m, tab.buf.as<CompactWord>(), reinterpret_cast<const uint32_t *>(tab.buf.as<uint8_t>() + words_bytes),
                       p.dst_words);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(dst->stream));          // (the tables go out of scope)
    return BIGSI_OK;
}

extern "C" int bigsi_hip_compact_columns(bigsi_hip_index *ix, const uint8_t *keep, uint64_t *new_num_cols)
{
    BIGSI_ENTER(ix);
    if (!ix || !keep) return fail(BIGSI_ERR_INVALID, "NULL argument");
    TRY(begin_rewrite(ix, "bigsi_hip_compact_columns", "their column count would go stale"));          // (a view is refused whatever `keep` says)
    const uint64_t kept = count_kept_columns(ix->n_cols, keep);
    if (kept < ix->n_cols) {          // (every column kept: the matrix stays as it is, byte for byte, and no table is built)
        const CompactPlan p = plan_compact_columns(ix->n_cols, keep, ix->m);
        TRY(compact_launch(ix, ix, p));
        ix->n_cols = p.kept;
    }
    if (new_num_cols) *new_num_cols = kept;
    return BIGSI_OK;
}

extern "C" int bigsi_hip_extract_columns(bigsi_hip_index *dst, const bigsi_hip_index *src, const uint8_t *keep)
{
    BIGSI_ENTER_DERIVE(dst, src);
    if (!keep) return fail(BIGSI_ERR_INVALID, "NULL argument");
    TRY(check_derive({"bigsi_hip_extract_columns", /*in_place*/ "bigsi_hip_compact_columns", /*rows_divide*/ false, /*same_hashes*/ false, /*into_empty*/ true}, dst, src));
    const CompactPlan p = plan_compact_columns(src->n_cols, keep, dst->m);
    TRY(begin_derive(dst, src, p.kept));
    TRY(compact_launch(dst, src, p));
    dst->n_cols = p.kept;
    return BIGSI_OK;
}

extern "C" int bigsi_hip_shrink_to_fit(bigsi_hip_index *ix)
{
    BIGSI_ENTER(ix);
    if (!ix) return fail(BIGSI_ERR_INVALID, "NULL index");
    const uint64_t ns = stride_for(std::max<uint64_t>(ix->n_cols, 1));
    if (ns >= ix->stride_words) return BIGSI_OK;          // (as bigsi_hip_reserve_cols: only a call that would really re-stride the matrix needs to own it)
    TRY(begin_rewrite(ix, "bigsi_hip_shrink_to_fit", "re-striding would move the matrix under them"));
    return replace_matrix(ix, ns, "bigsi_hip_shrink_to_fit");
}

// Column collapse (k_collapse_columns; tables, launch shape and destination window: plan_collapse_columns).  The tables live for this
// call only, like the compaction's: 4 bytes per source column and 8 per source word, 412 KB for 100 k columns.
extern "C" int bigsi_hip_collapse_columns_into(bigsi_hip_index *dst, const bigsi_hip_index *src, const uint32_t *group_of, uint64_t num_groups)
{
    BIGSI_ENTER_DERIVE(dst, src);
    if (!dst || !src || !group_of) return fail(BIGSI_ERR_INVALID, "NULL argument");
    if (num_groups == 0 || num_groups >= 0xFFFFFFFFull) return fail(BIGSI_ERR_INVALID, "num_groups %llu is not in [1, 2^32 - 1)", (unsigned long long)num_groups);
    TRY(check_derive({"bigsi_hip_collapse_columns_into", /*in_place*/ nullptr, /*rows_divide*/ false, /*same_hashes*/ true, /*into_empty*/ true}, dst, src));
    const uint64_t bad = collapse_first_bad(src->n_cols, group_of, num_groups);
    if (bad < src->n_cols)
        return fail(BIGSI_ERR_INVALID, "group_of[%llu] = %u is neither a group id below %llu nor BIGSI_COLLAPSE_DROPPED", (unsigned long long)bad, group_of[bad],
                    (unsigned long long)num_groups);
    const CollapsePlan p = plan_collapse_columns(src->n_cols, group_of, num_groups, dst->m);
    TRY(begin_derive(dst, src, num_groups));
    if (p.table_words > src->stride_words || round_up(p.dst_words, 2) > dst->stride_words || src->stride_words % kVec || dst->stride_words % kVec ||
        p.lds_bytes > kCollapseLdsBytes || p.image_words % 2 || p.grid == 0 || p.grid > 0x7FFFFFFFull)
        return fail(BIGSI_ERR_STATE, "internal: a collapse plan of %llu source and %llu destination words does not fit the row strides (%llu, %llu) or the LDS (%llu bytes)",
                    (unsigned long long)p.table_words, (unsigned long long)p.dst_words, (unsigned long long)src->stride_words,
                    (unsigned long long)dst->stride_words, (unsigned long long)p.lds_bytes);
    CallScratch tab;
    const uint64_t bit_bytes = std::max<uint64_t>(p.dst_bit.size() * 4, 16), live_bytes = std::max<uint64_t>(p.live.size() * 8, 16);
    TRY(tab.buf.reserve(bit_bytes + live_bytes));          // (bit_bytes is a multiple of 16: live is read 16 bytes at a time)
    if (!p.dst_bit.empty()) {
        HIP_TRY(hipMemcpyAsync(tab.buf.p, p.dst_bit.data(), p.dst_bit.size() * 4, hipMemcpyHostToDevice, dst->stream));
        HIP_TRY(hipMemcpyAsync(tab.buf.as<uint8_t>() + bit_bytes, p.live.data(), p.live.size() * 8, hipMemcpyHostToDevice, dst->stream));
    }
    hipLaunchKernelGGL(k_collapse_columns, dim3((unsigned)p.grid), dim3(p.block), (size_t)p.lds_bytes, dst->stream, src->d_index, src->stride_words, dst->d_index,
                       dst->stride_words, dst->m, tab.buf.as<uint32_t>(), reinterpret_cast<const uint64_t *>(tab.buf.as<uint8_t>() + bit_bytes), p.table_words,
                       p.dst_words, p.window_words, (uint32_t)p.image_words);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(dst->stream));          // (the tables go out of scope)
    dst->n_cols = num_groups;
    return BIGSI_OK;
}

// Consensus collapse (k_consensus_columns<field bits>; tables, field width, launch shape and destination window:
// plan_consensus_columns).  The tables live for this call only: the collapse's two and 4 bytes per destination column of thresholds.
template <int FIELD_BITS>
static void consensus_launch(bigsi_hip_index *dst, const bigsi_hip_index *src, const ConsensusPlan &p, const uint32_t *d_col, const uint64_t *d_live,
                             const uint32_t *d_need)
{
    hipLaunchKernelGGL(k_consensus_columns<FIELD_BITS>, dim3((unsigned)p.grid), dim3(p.block), (size_t)p.lds_bytes, dst->stream, src->d_index, src->stride_words,
                       dst->d_index, dst->stride_words, dst->m, d_col, d_live, d_need, p.table_words, p.dst_words, p.window_words, (uint32_t)p.image_words);
}

extern "C" int bigsi_hip_consensus_columns_into(bigsi_hip_index *dst, const bigsi_hip_index *src, const uint32_t *group_of, uint64_t num_groups,
                                                const uint32_t *min_members)
{
    BIGSI_ENTER_DERIVE(dst, src);
    if (!dst || !src || !group_of || !min_members) return fail(BIGSI_ERR_INVALID, "NULL argument");
    if (num_groups == 0 || num_groups >= 0xFFFFFFFFull) return fail(BIGSI_ERR_INVALID, "num_groups %llu is not in [1, 2^32 - 1)", (unsigned long long)num_groups);
    TRY(check_derive({"bigsi_hip_consensus_columns_into", /*in_place*/ nullptr, /*rows_divide*/ false, /*same_hashes*/ true, /*into_empty*/ true}, dst, src));
    const uint64_t bad = collapse_first_bad(src->n_cols, group_of, num_groups);
    if (bad < src->n_cols)
        return fail(BIGSI_ERR_INVALID, "group_of[%llu] = %u is neither a group id below %llu nor BIGSI_COLLAPSE_DROPPED", (unsigned long long)bad, group_of[bad],
                    (unsigned long long)num_groups);
    const uint64_t zero = consensus_first_zero(min_members, num_groups);
    if (zero < num_groups)
        return fail(BIGSI_ERR_INVALID, "min_members[%llu] is 0: a group keeps a bit that at least one member has (0 would mean an all-ones column)",
                    (unsigned long long)zero);
    const ConsensusPlan p = plan_consensus_columns(src->n_cols, group_of, num_groups, min_members, dst->m);
    TRY(begin_derive(dst, src, num_groups));
    const uint64_t field_max = p.field_bits == 32 ? 0xFFFFFFFFull : (1ull << p.field_bits) - 1;
    if (p.table_words > src->stride_words || round_up(p.dst_words, 2) > dst->stride_words || src->stride_words % kVec || dst->stride_words % kVec ||
        p.lds_bytes > kCollapseLdsBytes || p.window_words == 0 || p.window_words % 2 || p.image_words % (2 * p.field_bits) ||
        p.image_words < std::min<uint64_t>(p.window_words, round_up(p.dst_words, 2)) * p.field_bits || p.largest > field_max ||
        p.need.size() != round_up(p.dst_words, 2) * 64 || p.grid == 0 || p.grid > 0x7FFFFFFFull)
        return fail(BIGSI_ERR_STATE, "internal: a consensus plan of %llu source and %llu destination words at %u-bit fields does not fit the row strides (%llu, %llu) or the LDS (%llu bytes)",
                    (unsigned long long)p.table_words, (unsigned long long)p.dst_words, p.field_bits, (unsigned long long)src->stride_words,
                    (unsigned long long)dst->stride_words, (unsigned long long)p.lds_bytes);
    CallScratch tab;
    const uint64_t col_bytes = std::max<uint64_t>(p.dst_col.size() * 4, 16), live_bytes = std::max<uint64_t>(p.live.size() * 8, 16), need_bytes = p.need.size() * 4;
    TRY(tab.buf.reserve(col_bytes + live_bytes + need_bytes));          // (col_bytes and live_bytes are multiples of 16: live is read 16 bytes at a time)
    if (!p.dst_col.empty()) {
        HIP_TRY(hipMemcpyAsync(tab.buf.p, p.dst_col.data(), p.dst_col.size() * 4, hipMemcpyHostToDevice, dst->stream));
        HIP_TRY(hipMemcpyAsync(tab.buf.as<uint8_t>() + col_bytes, p.live.data(), p.live.size() * 8, hipMemcpyHostToDevice, dst->stream));
    }
    HIP_TRY(hipMemcpyAsync(tab.buf.as<uint8_t>() + col_bytes + live_bytes, p.need.data(), need_bytes, hipMemcpyHostToDevice, dst->stream));
    const uint32_t *d_col = tab.buf.as<uint32_t>();
    const uint64_t *d_live = reinterpret_cast<const uint64_t *>(tab.buf.as<uint8_t>() + col_bytes);
    const uint32_t *d_need = reinterpret_cast<const uint32_t *>(tab.buf.as<uint8_t>() + col_bytes + live_bytes);
    if (p.field_bits == 8) consensus_launch<8>(dst, src, p, d_col, d_live, d_need);
    else if (p.field_bits == 16) consensus_launch<16>(dst, src, p, d_col, d_live, d_need);
    else consensus_launch<32>(dst, src, p, d_col, d_live, d_need);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(dst->stream));          // (the tables go out of scope)
    dst->n_cols = num_groups;
    return BIGSI_OK;
}

// Pairwise popcounts (k_columns_to_planes, k_pair_popcount, k_pair_popcount_sum; chunks, slices and scratch: plan_pairwise; tables:
// pairwise_tables).  Two allocations that live for this call only: the scratch (tables | planes | partials) and the 64-bit device
// result.  Either may not fit beside a large index: BIGSI_ERR_NOMEM then, with nothing leaked and the runtime's sticky last-error
// slot clear, as in replace_matrix.
namespace {
struct PairScratch {
    void *scratch = nullptr, *result = nullptr;
    hipEvent_t ev[2] = {nullptr, nullptr};
    ~PairScratch()
    {
        hipError_t e;
        for (hipEvent_t v : ev)
            if (v) { e = hipEventDestroy(v); (void)e; }
        if (scratch) { e = hipFree(scratch); (void)e; }
        if (result) { e = hipFree(result); (void)e; }
    }
};
}  // namespace

static int pair_alloc(void **p, size_t bytes, const char *what)
{
    const hipError_t e = hipMalloc(p, bytes);
    if (e == hipSuccess) return BIGSI_OK;
    (void)hipGetLastError();
    *p = nullptr;
    return fail(e == hipErrorOutOfMemory ? BIGSI_ERR_NOMEM : BIGSI_ERR_HIP, "bigsi_hip_pairwise_popcounts: hipMalloc of %zu bytes for %s beside the matrix failed: %s", bytes,
                what, hipGetErrorString(e));
}

// with profiling on: the time of what was queued on the stream since `ev[0]` was recorded, added to *ms
static int pair_phase(bigsi_hip_index *ix, PairScratch &s, double *ms)
{
    HIP_TRY(hipGetLastError());
    if (!ix->profiling) return BIGSI_OK;
    float t = 0;
    HIP_TRY(hipEventRecord(s.ev[1], ix->stream));
    HIP_TRY(hipEventSynchronize(s.ev[1]));
    HIP_TRY(hipEventElapsedTime(&t, s.ev[0], s.ev[1]));
    *ms += t;
    HIP_TRY(hipEventRecord(s.ev[0], ix->stream));
    return BIGSI_OK;
}

extern "C" int bigsi_hip_pairwise_popcounts(bigsi_hip_index *ix, const uint32_t *cols_a, uint64_t na, const uint32_t *cols_b, uint64_t nb, uint64_t *out,
                                            uint64_t capacity)
{
    BIGSI_ENTER(ix);
    if (!ix || !cols_a || !out) return fail(BIGSI_ERR_INVALID, "NULL argument");
    if (na == 0 || (cols_b && nb == 0)) return fail(BIGSI_ERR_INVALID, "an empty list of columns");
    const bool symmetric = cols_b == nullptr;
    if (symmetric) nb = na;
    uint64_t bad = pairwise_first_bad(cols_a, na, ix->n_cols);
    if (bad < na)
        return fail(BIGSI_ERR_RANGE, "cols_a[%llu] = %u is not a column of the index [0,%llu)", (unsigned long long)bad, cols_a[bad], (unsigned long long)ix->n_cols);
    if (!symmetric && (bad = pairwise_first_bad(cols_b, nb, ix->n_cols)) < nb)
        return fail(BIGSI_ERR_RANGE, "cols_b[%llu] = %u is not a column of the index [0,%llu)", (unsigned long long)bad, cols_b[bad], (unsigned long long)ix->n_cols);
    const unsigned __int128 pairs = (unsigned __int128)na * nb;
    if (pairs > capacity) return fail(BIGSI_ERR_CAPACITY, "capacity %llu is below na x nb = %llu x %llu", (unsigned long long)capacity, (unsigned long long)na, (unsigned long long)nb);
    if (pairs > BIGSI_PAIRWISE_MAX_PAIRS)
        return fail(BIGSI_ERR_RANGE, "na x nb = %llu x %llu is above BIGSI_PAIRWISE_MAX_PAIRS (%llu)", (unsigned long long)na, (unsigned long long)nb, (unsigned long long)BIGSI_PAIRWISE_MAX_PAIRS);
    static_assert(kPairwiseMaxPairs == BIGSI_PAIRWISE_MAX_PAIRS, "the planner's bound is the header's");
    if (ix->m == 0) { memset(out, 0, na * nb * 8); return BIGSI_OK; }
    TRY(use_device(ix));

    const PairwiseTables t = pairwise_tables(cols_a, na, cols_b, nb);
    const uint64_t nua = t.plane_a.size(), nub = symmetric ? nua : t.plane_b.size(), distinct = t.bit.size(), nw = t.words.size();
    const PairwisePlan p = plan_pairwise(nua, nub, symmetric, ix->m, ix->stride_words);
    if (p.tiles > 0x7FFFFFFFull || p.slices > 65535 || distinct * p.chunk_words * 8 > p.plane_bytes || t.words.back() >= ix->stride_words)
        return fail(BIGSI_ERR_STATE, "internal: a pairwise plan of %llu tiles x %llu slices over %llu distinct columns does not fit a launch or its planes",
                    (unsigned long long)p.tiles, (unsigned long long)p.slices, (unsigned long long)distinct);
    // scratch: words | first | bit | plane_a | plane_b | map_a | map_b | planes | partials, every part on a 256-byte boundary
    const std::vector<uint32_t> *tabs[7] = {&t.words, &t.first, &t.bit, &t.plane_a, &t.plane_b, &t.map_a, &t.map_b};
    uint64_t off[9], at = 0;
    for (int k = 0; k < 7; k++) { off[k] = at; at += round_up(tabs[k]->size() * 4, 256); }
    off[7] = at; at += round_up(p.plane_bytes, 256);
    off[8] = at; at += round_up(p.partial_bytes, 256);
    PairScratch s;
    TRY(pair_alloc(&s.scratch, at, "the planes and partial counts"));
    TRY(pair_alloc(&s.result, na * nb * 8, "the result"));
    uint8_t *base = reinterpret_cast<uint8_t *>(s.scratch);
    for (int k = 0; k < 7; k++)
        if (!tabs[k]->empty()) HIP_TRY(hipMemcpyAsync(base + off[k], tabs[k]->data(), tabs[k]->size() * 4, hipMemcpyHostToDevice, ix->stream));
    const auto tab = [&](int k) { return reinterpret_cast<const uint32_t *>(base + off[k]); };
    const uint32_t *d_plane_b = symmetric ? tab(3) : tab(4), *d_map_b = symmetric ? tab(5) : tab(6);
    uint64_t *planes = reinterpret_cast<uint64_t *>(base + off[7]);
    uint32_t *partial = reinterpret_cast<uint32_t *>(base + off[8]);
    double ms[4] = {0, 0, 0, (double)p.chunks};
    if (ix->profiling) {
        HIP_TRY(hipEventCreate(&s.ev[0]));
        HIP_TRY(hipEventCreate(&s.ev[1]));
        HIP_TRY(hipEventRecord(s.ev[0], ix->stream));
    }
    const unsigned sum_grid = (unsigned)std::min<uint64_t>(ceil_div(na * nb, kBlock), 256 * 8 * 4);
    for (uint64_t c = 0; c < p.chunks; c++) {
        const uint64_t words = pairwise_chunk_words(p, c), slices = pairwise_chunk_slices(p, words);
        hipLaunchKernelGGL(k_columns_to_planes, dim3((unsigned)ceil_div(words, kBlock / 64)), dim3(kBlock), 0, ix->stream, ix->d_index, ix->stride_words, ix->m,
                           c * p.chunk_words * 64, words, tab(0), tab(1), tab(2), (uint32_t)nw, planes, p.chunk_words);
        TRY(pair_phase(ix, s, &ms[0]));
        hipLaunchKernelGGL(k_pair_popcount, dim3((unsigned)p.tiles, (unsigned)slices), dim3(kBlock), 0, ix->stream, planes, p.chunk_words, words, p.slice_words, tab(3),
                           (uint32_t)nua, d_plane_b, (uint32_t)nub, (uint32_t)p.tiles_j, symmetric ? 1u : 0u, partial);
        TRY(pair_phase(ix, s, &ms[1]));
        hipLaunchKernelGGL(k_pair_popcount_sum, dim3(sum_grid), dim3(kBlock), 0, ix->stream, partial, slices, (uint32_t)nua, (uint32_t)nub, tab(5), na, d_map_b, nb,
                           symmetric ? 1u : 0u, c ? 1u : 0u, reinterpret_cast<uint64_t *>(s.result));
        TRY(pair_phase(ix, s, &ms[2]));
    }
    HIP_TRY(hipMemcpyAsync(out, s.result, na * nb * 8, hipMemcpyDeviceToHost, ix->stream));
    HIP_TRY(hipStreamSynchronize(ix->stream));          // (the scratch goes out of scope)
    if (ix->profiling) memcpy(ix->pair_ms, ms, sizeof ms);
    return BIGSI_OK;
}

extern "C" int bigsi_hip_pairwise_phase_ms(bigsi_hip_index *ix, double ms[4])
{
    BIGSI_ENTER(ix);
    if (!ix || !ms) return fail(BIGSI_ERR_INVALID, "NULL argument");
    memcpy(ms, ix->pair_ms, sizeof ix->pair_ms);
    return BIGSI_OK;
}

// Row folding (k_fold_rows; launch shape: plan_fold_rows).  `dst` may be `src` (in place: see the kernel); factors below kFoldLoads
// have a kernel of their own (the factor is a compile-time constant there), every other factor runs the generic one.
template <int D>
static void fold_launch_as(const FoldPlan &p, hipStream_t st, const uint64_t *src, uint64_t src_stride, uint64_t *dst, uint64_t dst_stride, uint64_t m_dst,
                           uint64_t factor, uint64_t words, uint64_t tail_mask)
{
    hipLaunchKernelGGL((k_fold_rows<D, kFoldNtLoads>), dim3((unsigned)p.grid), dim3(p.block), 0, st, src, src_stride, dst, dst_stride, m_dst, factor, words,
                       tail_mask, p.rows_per_block, (uint32_t)p.seg_groups);
}

static int fold_launch(bigsi_hip_index *dst, const bigsi_hip_index *src, uint64_t m_dst, uint64_t factor, uint64_t n_cols)
{
    const uint64_t words = ceil_div(n_cols, 64);
    if (words > src->stride_words || words > dst->stride_words || src->stride_words % kVec || dst->stride_words % kVec)
        return fail(BIGSI_ERR_STATE, "internal: %llu column words do not fit the row strides (%llu, %llu)", (unsigned long long)words,
                    (unsigned long long)src->stride_words, (unsigned long long)dst->stride_words);
    // the columns of the last word that exist, in the row format: column c of a word at bit 8 (c / 8) + 7 - c % 8
    uint64_t tail_mask = ~0ull;
    if (n_cols & 63) {
        tail_mask = 0;
        for (uint32_t c = 0; c < (n_cols & 63); c++) tail_mask |= 1ull << bit_of_col(c);
    }
    const FoldPlan p = plan_fold_rows(m_dst, factor, dst->stride_words);
    if (p.grid > 0x7FFFFFFFull) return fail(BIGSI_ERR_INVALID, "internal: a fold grid of %llu workgroups", (unsigned long long)p.grid);
    hipStream_t st = dst->stream;
#define FOLD_AS(D) fold_launch_as<D>(p, st, src->d_index, src->stride_words, dst->d_index, dst->stride_words, m_dst, factor, words, tail_mask)
    switch (factor) {
    case 1: FOLD_AS(1); break;
    case 2: FOLD_AS(2); break;
    case 3: FOLD_AS(3); break;
    case 4: FOLD_AS(4); break;
    case 5: FOLD_AS(5); break;
    case 6: FOLD_AS(6); break;
    case 7: FOLD_AS(7); break;
    default: FOLD_AS(0); break;
    }
#undef FOLD_AS
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(st));
    return BIGSI_OK;
}

extern "C" int bigsi_hip_fold_rows(bigsi_hip_index *ix, uint64_t factor, uint64_t *new_num_rows)
{
    BIGSI_ENTER(ix);
    if (!ix) return fail(BIGSI_ERR_INVALID, "NULL index");
    if (factor == 0 || ix->m % factor)
        return fail(BIGSI_ERR_INVALID, "fold factor %llu does not divide num_rows %llu", (unsigned long long)factor, (unsigned long long)ix->m);
    if (factor > 1) {          // (factor 1: the index stays as it is, and nothing is touched)
        TRY(begin_rewrite(ix, "bigsi_hip_fold_rows", "their row count would go stale"));
        const uint64_t m_dst = ix->m / factor;
        TRY(fold_launch(ix, ix, m_dst, factor, ix->n_cols));
        ix->m = m_dst;          // (alloc_rows stays: bigsi_hip_trim_rows gives the rows behind m back)
    }
    if (new_num_rows) *new_num_rows = ix->m;
    return BIGSI_OK;
}

extern "C" int bigsi_hip_fold_rows_into(bigsi_hip_index *dst, const bigsi_hip_index *src)
{
    BIGSI_ENTER_DERIVE(dst, src);
    TRY(check_derive({"bigsi_hip_fold_rows_into", /*in_place*/ "bigsi_hip_fold_rows", /*rows_divide*/ true, /*same_hashes*/ true, /*into_empty*/ true}, dst, src));
    TRY(begin_derive(dst, src, src->n_cols));
    TRY(fold_launch(dst, src, dst->m, src->m / dst->m, src->n_cols));
    dst->n_cols = src->n_cols;
    return BIGSI_OK;
}

extern "C" int bigsi_hip_trim_rows(bigsi_hip_index *ix)
{
    BIGSI_ENTER(ix);
    if (!ix) return fail(BIGSI_ERR_INVALID, "NULL index");
    TRY(bigsi_writable(ix));          // (a handle that does not own the matrix does not know its allocation: refused whatever there is to gain)
    if (ix->alloc_rows <= ix->m) return BIGSI_OK;
    TRY(begin_rewrite(ix, "bigsi_hip_trim_rows", "trimming would move the matrix under them"));
    return replace_matrix(ix, ix->stride_words, "bigsi_hip_trim_rows");          // rows [0, m) are the front of the old allocation, at the same stride
}

static int check_offsets(const uint64_t *offsets, uint32_t n_seqs)
{
    for (uint32_t i = 0; i < n_seqs; i++) {
        if (offsets[i + 1] < offsets[i]) return fail(BIGSI_ERR_INVALID, "offsets must be non-decreasing");
        if (offsets[i + 1] - offsets[i] > 0xFFFFFFF0ull) return fail(BIGSI_ERR_INVALID, "sequence %u longer than 2^32-16 bytes", i);
    }
    return BIGSI_OK;
}

extern "C" int bigsi_hip_insert_kmers(bigsi_hip_index *ix, uint64_t col, const char *seqs, const uint64_t *offsets, uint32_t n_seqs, uint32_t k)
{
    BIGSI_ENTER(ix);
    TRY(bigsi_writable(ix));
    if (!ix || !offsets || (n_seqs && !seqs && offsets[n_seqs] > offsets[0])) return fail(BIGSI_ERR_INVALID, "NULL argument");
    if (k == 0) return fail(BIGSI_ERR_INVALID, "k must be > 0");
    if (col >= ix->n_cols) return fail(BIGSI_ERR_RANGE, "column %llu >= num_cols %llu", (unsigned long long)col, (unsigned long long)ix->n_cols);
    if (n_seqs == 0) return BIGSI_OK;
    TRY(check_offsets(offsets, n_seqs));
    TRY(use_device(ix));
    TRY(quiesce_index(ix));
    const uint64_t base = offsets[0], nbytes = offsets[n_seqs] - base;
    std::vector<uint64_t> rel(n_seqs + 1);
    for (uint32_t i = 0; i <= n_seqs; i++) rel[i] = offsets[i] - base;
    TRY(ix->stage.reserve(std::max<uint64_t>(nbytes, 1)));
    TRY(ix->stage_ids.reserve((n_seqs + 1) * 8ull));
    if (nbytes) HIP_TRY(hipMemcpyAsync(ix->stage.p, seqs + base, nbytes, hipMemcpyHostToDevice, ix->stream));
    HIP_TRY(hipMemcpyAsync(ix->stage_ids.p, rel.data(), (n_seqs + 1) * 8ull, hipMemcpyHostToDevice, ix->stream));
    hipLaunchKernelGGL(k_insert_kmers, dim3(n_seqs), dim3(kBlock), 0, ix->stream, ix->d_index, ix->stride_words, ix->m, ix->h, col,
                       ix->stage.as<char>(), ix->stage_ids.as<uint64_t>(), k);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(ix->stream));   // rel[] and the staging buffers go out of scope
    return BIGSI_OK;
}

extern "C" int bigsi_hip_fill_synthetic(bigsi_hip_index *ix, uint64_t seed, uint64_t shard, uint32_t and_draws)
{
    BIGSI_ENTER(ix);
    TRY(bigsi_writable(ix));
    if (!ix) return fail(BIGSI_ERR_INVALID, "NULL index");
    if (and_draws == 0 || and_draws > 8) return fail(BIGSI_ERR_INVALID, "and_draws must be in [1,8]");
    TRY(use_device(ix));
    TRY(quiesce_index(ix));
    hipLaunchKernelGGL(k_fill_synth, dim3(256 * 16), dim3(kBlock), 0, ix->stream, ix->d_index, ix->m, ix->stride_words, ix->n_cols, seed, shard, and_draws);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(ix->stream));
    return BIGSI_OK;
}

extern "C" int bigsi_hip_bloom(int device, const char *kmers, uint64_t u, uint32_t k, uint64_t m, uint32_t h, uint32_t flags, uint8_t *out)
{
    if (!out || (u && !kmers)) return fail(BIGSI_ERR_INVALID, "NULL argument");
    if (k == 0 || m == 0 || h == 0) return fail(BIGSI_ERR_INVALID, "k, m and h must be > 0");
    HIP_TRY(hipSetDevice(device));
    const uint64_t nwords = ceil_div(m, 32), nb = ceil_div(m, 8);
    uint32_t *d_bits = nullptr;
    char *d_km = nullptr;
    HIP_TRY(hipMalloc((void **)&d_bits, nwords * 4));
    hipError_t e = hipMemset(d_bits, 0, nwords * 4);
    if (e == hipSuccess && u) {
        e = hipMalloc((void **)&d_km, u * k);
        if (e == hipSuccess) e = hipMemcpy(d_km, kmers, u * k, hipMemcpyHostToDevice);
        if (e == hipSuccess) {
            const unsigned grid = (unsigned)std::min<uint64_t>(ceil_div(u, kBlock), 256 * 8);
            hipLaunchKernelGGL(k_bloom, dim3(grid), dim3(kBlock), 0, 0, d_bits, m, h, d_km, u, k, (flags & BIGSI_BLOOM_RAW) != 0);
            e = hipGetLastError();
        }
    }
    if (e == hipSuccess) e = hipMemcpy(out, d_bits, nb, hipMemcpyDeviceToHost);   // little-endian words == byte order
    hipError_t e2 = hipFree(d_bits); (void)e2;
    if (d_km) e2 = hipFree(d_km);
    if (e != hipSuccess) return fail(BIGSI_ERR_HIP, "bigsi_hip_bloom: %s", hipGetErrorString(e));
    return BIGSI_OK;
}

// ------------------------------------------------------------------------------ profiling events
int bigsi_ev_begin(bigsi_hip_index *ix, EventPair *p, hipStream_t st, bool row_and)
{
    if (!st) st = ix->stream;
    *p = EventPair{};
    if (!ix->profiling || (ix->profiling == 2 && !row_and)) return BIGSI_OK;
    if (ix->prof_every > 1 && row_and && (ix->prof_tick++ % ix->prof_every) != 0) return BIGSI_OK;      // sampled: this run goes untimed
    if (ix->ev_free.empty()) {
        EventPair n;
        HIP_TRY(hipEventCreate(&n.a));
        HIP_TRY(hipEventCreate(&n.b));
        ix->ev_free.push_back(n);
    }
    *p = ix->ev_free.back();
    ix->ev_free.pop_back();
    HIP_TRY(hipEventRecord(p->a, st));
    return BIGSI_OK;
}

int bigsi_ev_end(bigsi_hip_index *ix, EventPair *p, std::vector<EventPair> &dst, hipStream_t st, uint32_t launches)
{
    if (&dst == &ix->ev_and) ix->and_total += launches;
    if (!p->a) return BIGSI_OK;          // not being timed
    if (!st) st = ix->stream;
    HIP_TRY(hipEventRecord(p->b, st));
    p->launches = launches;
    dst.push_back(*p);
    return BIGSI_OK;
}

extern "C" int bigsi_hip_set_profiling(bigsi_hip_index *ix, int on)
{
    BIGSI_ENTER(ix);
    if (!ix) return fail(BIGSI_ERR_INVALID, "NULL index");
    ix->profiling = on >= 2 ? 2 : (on != 0);
    ix->prof_every = on > 2 ? (uint32_t)on : 1u;
    ix->prof_tick = 0;
    return BIGSI_OK;
}

extern "C" int bigsi_hip_stats(bigsi_hip_index *ix, bigsi_hip_stats_t *out, int reset)
{
    BIGSI_ENTER(ix);
    if (!ix || !out) return fail(BIGSI_ERR_INVALID, "NULL argument");
    TRY(use_device(ix));
    TRY(quiesce_index(ix));
    HIP_TRY(hipStreamSynchronize(ix->pre_stream));
    HIP_TRY(hipStreamSynchronize(ix->stream));
    auto sum = [&](std::vector<EventPair> &v, uint64_t *n, double *ms) -> int {
        *n = 0;
        *ms = 0;
        for (auto &p : v) {
            *n += p.launches;
            float t = 0;
            HIP_TRY(hipEventSynchronize(p.b));      // (pairs recorded on a communicator's or a caller's stream)
            HIP_TRY(hipEventElapsedTime(&t, p.a, p.b));
            *ms += t;
        }
        return BIGSI_OK;
    };
    TRY(sum(ix->ev_and, &out->and_launches, &out->and_ms));
    TRY(sum(ix->ev_km, &out->kmerize_launches, &out->kmerize_ms));
    TRY(sum(ix->ev_cp, &out->compact_launches, &out->compact_ms));
    TRY(sum(ix->ev_pr, &out->presence_launches, &out->presence_ms));
    TRY(sum(ix->ev_tr, &out->transpose_launches, &out->transpose_ms));
    TRY(sum(ix->ev_ex, &out->exchange_launches, &out->exchange_ms));
    out->presence_bytes = ix->presence_bytes;
    out->index_contiguous = 0;
    out->and_launches_total = ix->and_total;
    out->read_launches_repeated = ix->fused_repeats;
    if (reset) {
        recycle_events(ix);
        ix->presence_bytes = 0;
        ix->and_total = 0;
        ix->fused_repeats = 0;
    }
    return BIGSI_OK;
}

// MEASUREMENT: bare row streams over this index's own matrix (k_probe_rows): GB/s of `n_queries` lists of `rows_per_query`
// rows each, uniform random (sorted = 0) or ascending (1), in launches of `wgs` four-wavefront workgroups (0: as the library
// sizes its own row-AND launches -- the smallest multiple of 256 workgroups with >= 1600 live wavefronts); median launch of
// `reps` passes after one warm pass, HIP events on the index stream.
extern "C" int bigsi_hip_probe_rows(bigsi_hip_index *ix, uint32_t rows_per_query, uint32_t n_queries, uint32_t sorted, uint32_t wgs, uint32_t reps,
                                    double *gbps, double *launch_ms)
{
    BIGSI_ENTER(ix);
    if (!ix || !gbps) return fail(BIGSI_ERR_INVALID, "NULL argument");
    if (rows_per_query == 0 || n_queries == 0 || reps == 0) return fail(BIGSI_ERR_INVALID, "rows_per_query, n_queries and reps must be > 0");
    if (ix->n_cols == 0) return fail(BIGSI_ERR_STATE, "index has no columns");
    TRY(use_device(ix));
    TRY(quiesce_index(ix));
    const uint32_t wv = (uint32_t)ix->wv(), segs = (uint32_t)ceil_div(wv, 64 * kVec), live = (uint32_t)ceil_div(wv, 64 * kVec);
    if (wgs == 0) wgs = (uint32_t)round_up(ceil_div(1600ull * ceil_div(segs, 4), live), 256);
    // as many LIVE wavefronts per launch as a row-AND launch of `wgs` workgroups has (there a query's last workgroup is partly empty)
    const uint32_t q_per_launch = std::max<uint32_t>(wgs / (uint32_t)ceil_div(segs, 4), 1);
    if (n_queries < 2 * q_per_launch) n_queries = 2 * q_per_launch;
    DevBuf ids, out;
    int rc = ids.reserve((size_t)n_queries * rows_per_query * 8);
    if (rc == BIGSI_OK) rc = out.reserve((size_t)q_per_launch * segs * 64 * 16);
    std::vector<float> ms;
    hipEvent_t e0 = nullptr, e1 = nullptr;
    auto body = [&]() -> int {
        HIP_TRY(hipEventCreate(&e0));
        HIP_TRY(hipEventCreate(&e1));
        hipLaunchKernelGGL(k_probe_ids, dim3(1024), dim3(kBlock), 0, ix->stream, ids.as<uint64_t>(), (uint64_t)n_queries, rows_per_query, ix->m, sorted, 0x5EEDull + sorted);
        HIP_TRY(hipGetLastError());
        for (uint32_t rep = 0; rep <= reps; rep++)
            for (uint32_t q0 = 0; q0 + q_per_launch <= n_queries; q0 += q_per_launch) {
                const uint32_t waves = q_per_launch * segs, blocks = (uint32_t)ceil_div(waves, 4);
                HIP_TRY(hipEventRecord(e0, ix->stream));
                hipLaunchKernelGGL(k_probe_rows, dim3(blocks), dim3(kBlock), 0, ix->stream, ix->d_index, ix->stride_words, wv, ids.as<uint64_t>(), rows_per_query, segs,
                                   q0, q0 + q_per_launch, reinterpret_cast<u64x2 *>(out.p));
                HIP_TRY(hipGetLastError());
                HIP_TRY(hipEventRecord(e1, ix->stream));
                HIP_TRY(hipEventSynchronize(e1));
                float t = 0;
                HIP_TRY(hipEventElapsedTime(&t, e0, e1));
                if (rep) ms.push_back(t);
            }
        return BIGSI_OK;
    };
    if (rc == BIGSI_OK) rc = body();
    hipError_t e = hipSuccess;
    if (e0) e = hipEventDestroy(e0);
    if (e1) e = hipEventDestroy(e1);
    (void)e;
    ids.release();
    out.release();
    if (rc != BIGSI_OK) return rc;
    std::sort(ms.begin(), ms.end());
    const double med = ms[ms.size() / 2];
    *gbps = (double)q_per_launch * rows_per_query * wv * 8.0 / (med * 1e-3) / 1e9;
    if (launch_ms) *launch_ms = med;
    return BIGSI_OK;
}

// ------------------------------------------------------------------------------ batches
static uint64_t pow2_at_least(uint64_t x)
{
    uint64_t p = 2;
    while (p < x) p <<= 1;
    return p;
}

// (re)load a batch object with sequences: host-side prefix arrays, grow-only device buffers, H2D copies
// num_kmers | num_unique | min_kmers of the batch's n_seqs sequences, side by side in b->uniq (host_counts: one download)
static void point_uniq(bigsi_hip_batch *b)
{
    uint32_t *u = b->uniq.as<uint32_t>();
    b->num_kmers.point(u, b->n_seqs * 4ull);
    b->num_unique.point(u + b->n_seqs, b->n_seqs * 4ull);
    b->min_kmers.point(u + 2ull * b->n_seqs, b->n_seqs * 4ull);
}

static int pinned_reserve(void **p, size_t *cap, size_t bytes);
static int export_wait(bigsi_hip_batch *b);

// `deferred`: the offset tables and the sequences are staged in pinned memory the batch owns and go up at the start of the next
// run, on the stream that run uses -- no copy, no synchronisation here (the one-call and streaming entry points: a call is then
// one asynchronous upload, the kernels, one export kernel and ONE wait).  Otherwise (create / reload) the copy is made now on
// the upload stream and waited for.
static int batch_load(bigsi_hip_batch *b, const char *seqs, const uint64_t *offsets, uint32_t n_seqs, uint32_t k, bool deferred = false)
{
    bigsi_hip_index *ix = b->ix;
    b->upload_deferred = false;
    b->zero_copy = false;
    const uint64_t base = offsets[0], nbytes = offsets[n_seqs] - base;
    b->n_seqs = n_seqs;
    b->k = k;
    b->ran = b->compacted = b->host_counts_valid = false;
    b->g_src = nullptr;
    b->max_pos = b->max_len = 0;
    b->seq_off.resize(n_seqs + 1);
    b->pos_off.resize(n_seqs + 1);
    b->tab_off.resize(n_seqs + 1);
    b->pos_off[0] = b->tab_off[0] = 0;
    for (uint32_t i = 0; i <= n_seqs; i++) b->seq_off[i] = offsets[i] - base;
    for (uint32_t i = 0; i < n_seqs; i++) {
        const uint64_t len = b->seq_off[i + 1] - b->seq_off[i];
        const uint64_t n = len >= k ? len - k + 1 : 0;
        b->pos_off[i + 1] = b->pos_off[i] + n;
        b->tab_off[i + 1] = b->tab_off[i] + pow2_at_least(2 * n);
        b->max_pos = std::max(b->max_pos, n);
        b->max_len = std::max(b->max_len, len);
    }
    b->total_pos = b->pos_off[n_seqs];
    const uint64_t T = std::max<uint64_t>(b->total_pos, 1);
    int rc = BIGSI_OK;
    auto R = [&](DevBuf &d, size_t bytes) { if (rc == BIGSI_OK) rc = d.reserve(bytes); };
    // upload arena: [seq_off | pos_off | tab_off | sequence bytes]; the three offset tables go up as ONE copy, together with the
    // sequences when those are short (a batch of reads: one copy instead of four), else the sequences straight from the caller
    const size_t ob = (n_seqs + 1) * 8ull;
    R(b->upload, 3 * ob + std::max<uint64_t>(nbytes, 1));
    R(b->first_pos, T * 4);
    R(b->pos_unique, T * 4);
    R(b->tmp, T * 4);
    R(b->rep, T * 4);
    R(b->rows, T * ix->h * 8);
    R(b->uniq, 3ull * n_seqs * 4);
    if (rc == BIGSI_OK) {
        uint8_t *u = b->upload.as<uint8_t>();
        b->d_seq_off.point(u, ob);
        b->d_pos_off.point(u + ob, ob);
        b->d_tab_off.point(u + 2 * ob, ob);
        b->seqs.point(u + 3 * ob, std::max<uint64_t>(nbytes, 1));
        point_uniq(b);
    }
    auto H2D = [&](void *dst, const void *src, size_t bytes) {
        if (rc == BIGSI_OK && bytes) {
            hipError_t e = hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, ix->pre_stream);
            if (e != hipSuccess) rc = fail(BIGSI_ERR_HIP, "H2D copy: %s", hipGetErrorString(e));
        }
    };
    if (deferred && rc == BIGSI_OK) {
        const size_t bytes = 3 * ob + nbytes;
        rc = pinned_reserve(&b->pin_up, &b->pin_up_cap, bytes);
        if (rc != BIGSI_OK) return rc;
        uint8_t *h = static_cast<uint8_t *>(b->pin_up);
        memcpy(h, b->seq_off.data(), ob);
        memcpy(h + ob, b->pos_off.data(), ob);
        memcpy(h + 2 * ob, b->tab_off.data(), ob);
        if (nbytes) memcpy(h + 3 * ob, seqs + base, nbytes);
        b->pin_up_bytes = bytes;
        b->upload_deferred = true;
        b->pos_query_loaded = false;
        return BIGSI_OK;
    }
    const bool packed = nbytes <= (64u << 10);
    b->h_upload.resize(3 * ob + (packed ? nbytes : 0));
    memcpy(b->h_upload.data(), b->seq_off.data(), ob);
    memcpy(b->h_upload.data() + ob, b->pos_off.data(), ob);
    memcpy(b->h_upload.data() + 2 * ob, b->tab_off.data(), ob);
    if (packed && nbytes) memcpy(b->h_upload.data() + 3 * ob, seqs + base, nbytes);
    H2D(b->upload.p, b->h_upload.data(), b->h_upload.size());
    if (!packed) H2D(b->seqs.p, seqs + base, nbytes);
    b->pos_query_loaded = false;
    if (rc == BIGSI_OK) {
        hipError_t e = hipStreamSynchronize(ix->pre_stream);  // the host vectors above are read by the copies
        if (e != hipSuccess) rc = fail(BIGSI_ERR_HIP, "sync: %s", hipGetErrorString(e));
    }
    return rc;
}

// host-side wait for everything queued on behalf of this batch (its K1 on the pre stream, K2-K4 on the index stream up to
// `done`, gathered compaction on the gather stream)
static int batch_quiesce(bigsi_hip_batch *b)
{
    if (b->idle) return BIGSI_OK;      // its last export was collected and nothing has been queued since
    if (b->done_stale && !b->dirty && b->run_stream) HIP_TRY(hipStreamSynchronize(b->run_stream));
    if (b->dirty) {
        HIP_TRY(hipStreamSynchronize(b->ix->pre_stream));
        HIP_TRY(hipStreamSynchronize(b->ix->stream));
        TRY(quiesce_reads(b->ix));
        b->dirty = false;
    } else if (b->done && !b->done_stale) {
        HIP_TRY(hipEventSynchronize(b->done));
    }
    if (b->g_done) HIP_TRY(hipEventSynchronize(b->g_done));
    if (b->job.done && b->job.device_work) HIP_TRY(hipEventSynchronize(b->job.done));      // a K5 / K6 request still reading this batch's arrays
    return BIGSI_OK;
}

static int check_batch_args(bigsi_hip_index *ix, const char *seqs, const uint64_t *offsets, uint32_t n_seqs, uint32_t k)
{
    if (!ix || !offsets) return fail(BIGSI_ERR_INVALID, "NULL argument");
    if (n_seqs == 0) return fail(BIGSI_ERR_INVALID, "a batch needs at least one sequence");
    if (k == 0) return fail(BIGSI_ERR_INVALID, "k must be > 0");
    TRY(check_offsets(offsets, n_seqs));
    if (offsets[n_seqs] - offsets[0] && !seqs) return fail(BIGSI_ERR_INVALID, "seqs is NULL");
    return BIGSI_OK;
}

extern "C" int bigsi_hip_batch_create(bigsi_hip_index *ix, const char *seqs, const uint64_t *offsets, uint32_t n_seqs, uint32_t k, bigsi_hip_batch **out)
{
    BIGSI_ENTER(ix);
    if (!out) return fail(BIGSI_ERR_INVALID, "out is NULL");
    *out = nullptr;
    TRY(check_batch_args(ix, seqs, offsets, n_seqs, k));
    TRY(use_device(ix));
    bigsi_hip_batch *b = new (std::nothrow) bigsi_hip_batch();
    if (!b) return fail(BIGSI_ERR_NOMEM, "host allocation failed");
    b->ix = ix;
    int rc = batch_load(b, seqs, offsets, n_seqs, k);
    if (rc != BIGSI_OK) { bigsi_hip_batch_destroy(b); return rc; }
    *out = b;
    return BIGSI_OK;
}

extern "C" int bigsi_hip_batch_create_elements(bigsi_hip_index *ix, const char *blob, const uint64_t *elem_offsets, const uint64_t *seq_elem_offsets,
                                               const uint32_t *pos_unique, const uint64_t *seq_pos_offsets, uint32_t n_seqs, bigsi_hip_batch **out)
{
    BIGSI_ENTER(ix);
    if (!out) return fail(BIGSI_ERR_INVALID, "out is NULL");
    *out = nullptr;
    if (!ix || !elem_offsets || !seq_elem_offsets || !seq_pos_offsets) return fail(BIGSI_ERR_INVALID, "NULL argument");
    if (n_seqs == 0) return fail(BIGSI_ERR_INVALID, "a batch needs at least one sequence");
    const uint64_t e_base = seq_elem_offsets[0], n_elems = seq_elem_offsets[n_seqs] - e_base;
    const uint64_t p_base = seq_pos_offsets[0], n_pos = seq_pos_offsets[n_seqs] - p_base;
    if (n_pos && !pos_unique) return fail(BIGSI_ERR_INVALID, "pos_unique is NULL");
    if (n_pos > 0xFFFFFFF0ull) return fail(BIGSI_ERR_INVALID, "too many k-mer positions");
    const uint64_t b_base = elem_offsets[e_base], n_bytes = elem_offsets[e_base + n_elems] - b_base;
    if (n_bytes && !blob) return fail(BIGSI_ERR_INVALID, "blob is NULL");
    TRY(use_device(ix));
    bigsi_hip_batch *b = new (std::nothrow) bigsi_hip_batch();
    if (!b) return fail(BIGSI_ERR_NOMEM, "host allocation failed");
    b->ix = ix;
    b->n_seqs = n_seqs;
    b->k = 0;
    b->elements = true;
    b->pos_off.resize(n_seqs + 1);
    b->seq_off.resize(n_elems + 1);              // element byte offsets (relative)
    std::vector<uint64_t> eso(n_seqs + 1);
    std::vector<uint32_t> first(std::max<uint64_t>(n_pos, 1)), rep(std::max<uint64_t>(n_pos, 1));
    int rc = BIGSI_OK;
    for (uint64_t e = 0; e <= n_elems && rc == BIGSI_OK; e++) {
        if (e && elem_offsets[e_base + e] < elem_offsets[e_base + e - 1]) rc = fail(BIGSI_ERR_INVALID, "elem_offsets must be non-decreasing");
        b->seq_off[e] = elem_offsets[e_base + e] - b_base;
    }
    for (uint32_t i = 0; i <= n_seqs; i++) {
        b->pos_off[i] = seq_pos_offsets[i] - p_base;
        eso[i] = seq_elem_offsets[i] - e_base;
    }
    for (uint32_t i = 0; i < n_seqs && rc == BIGSI_OK; i++) {
        if (b->pos_off[i + 1] < b->pos_off[i] || eso[i + 1] < eso[i]) { rc = fail(BIGSI_ERR_INVALID, "offsets must be non-decreasing"); break; }
        const uint64_t n = b->pos_off[i + 1] - b->pos_off[i], u = eso[i + 1] - eso[i];
        if (u > n) { rc = fail(BIGSI_ERR_INVALID, "sequence %u lists %llu unique k-mers for %llu positions", i, (unsigned long long)u, (unsigned long long)n); break; }
        const uint32_t *pu = pos_unique + p_base + b->pos_off[i];
        uint32_t *fp = first.data() + b->pos_off[i], *rp = rep.data() + b->pos_off[i];
        for (uint64_t j = 0; j < u; j++) fp[j] = 0xFFFFFFFFu;
        for (uint64_t t = 0; t < n && rc == BIGSI_OK; t++) {
            if (pu[t] >= u) rc = fail(BIGSI_ERR_RANGE, "pos_unique[%llu] of sequence %u is %u, beyond its %llu unique k-mers", (unsigned long long)t, i, pu[t], (unsigned long long)u);
            else if (fp[pu[t]] == 0xFFFFFFFFu) fp[pu[t]] = (uint32_t)t;
        }
        for (uint64_t j = 0; j < u && rc == BIGSI_OK; j++)
            if (fp[j] == 0xFFFFFFFFu) rc = fail(BIGSI_ERR_INVALID, "unique k-mer %llu of sequence %u occurs at no position", (unsigned long long)j, i);
        for (uint64_t t = 0; t < n && rc == BIGSI_OK; t++) rp[t] = fp[pu[t]];
        b->max_pos = std::max(b->max_pos, n);
    }
    b->total_pos = n_pos;
    const uint64_t T = std::max<uint64_t>(n_pos, 1);
    auto R = [&](DevBuf &d, size_t bytes) { if (rc == BIGSI_OK) rc = d.reserve(bytes); };
    R(b->seqs, std::max<uint64_t>(n_bytes, 1));
    R(b->d_seq_off, (n_elems + 1) * 8);
    R(b->elem_seq_off, (n_seqs + 1) * 8ull);
    R(b->d_pos_off, (n_seqs + 1) * 8ull);
    R(b->first_pos, T * 4);
    R(b->pos_unique, T * 4);
    R(b->rep, T * 4);
    R(b->rows, T * ix->h * 8);
    R(b->uniq, 3ull * n_seqs * 4);
    if (rc == BIGSI_OK) point_uniq(b);
    auto H2D = [&](void *dst, const void *src, size_t bytes) {
        if (rc == BIGSI_OK && bytes) {
            hipError_t e = hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, ix->pre_stream);
            if (e != hipSuccess) rc = fail(BIGSI_ERR_HIP, "H2D copy: %s", hipGetErrorString(e));
        }
    };
    H2D(b->seqs.p, blob ? blob + b_base : nullptr, n_bytes);
    H2D(b->d_seq_off.p, b->seq_off.data(), (n_elems + 1) * 8);
    H2D(b->elem_seq_off.p, eso.data(), (n_seqs + 1) * 8ull);
    H2D(b->d_pos_off.p, b->pos_off.data(), (n_seqs + 1) * 8ull);
    H2D(b->first_pos.p, first.data(), n_pos * 4);
    H2D(b->pos_unique.p, pos_unique ? pos_unique + p_base : nullptr, n_pos * 4);
    H2D(b->rep.p, rep.data(), n_pos * 4);
    if (rc == BIGSI_OK) {
        hipError_t e = hipStreamSynchronize(ix->pre_stream);
        if (e != hipSuccess) rc = fail(BIGSI_ERR_HIP, "sync: %s", hipGetErrorString(e));
    }
    if (rc != BIGSI_OK) {
        char keep[1024];
        snprintf(keep, sizeof keep, "%s", bigsi_hip_last_error());
        bigsi_hip_batch_destroy(b);
        return fail(rc, "%s", keep);
    }
    *out = b;
    return BIGSI_OK;
}

extern "C" int bigsi_hip_batch_reload(bigsi_hip_batch *b, const char *seqs, const uint64_t *offsets, uint32_t n_seqs, uint32_t k)
{
    BIGSI_ENTER(b ? b->ix : nullptr);
    if (!b) return fail(BIGSI_ERR_INVALID, "NULL batch");
    if (b->elements) return fail(BIGSI_ERR_STATE, "a batch of explicit k-mers cannot be reloaded: create a new one");
    TRY(check_batch_args(b->ix, seqs, offsets, n_seqs, k));
    TRY(use_device(b->ix));
    // only THIS batch's earlier work has to be over before its buffers are rewritten: other batches may still be running
    TRY(batch_quiesce(b));
    return batch_load(b, seqs, offsets, n_seqs, k);
}

extern "C" int bigsi_hip_batch_destroy(bigsi_hip_batch *b)
{
    BusyGuard busy_guard_(b ? b->ix : nullptr, /*wait=*/true);
    if (!b) return BIGSI_OK;
    hipError_t e = hipSetDevice(b->ix->device);
    e = hipStreamSynchronize(b->ix->pre_stream);
    e = hipStreamSynchronize(b->ix->stream);
    if (b->done) e = hipEventSynchronize(b->done);           // a run on one of the read streams
    if (b->exp_serial && b->exp_stream) e = hipStreamSynchronize(b->exp_stream);      // an export still writing into pin_out
    if (b->gstream && b->g_done) e = hipEventSynchronize(b->g_done);
    (void)e;
    b->planes.release();
    for (DevBuf *d : {&b->uniq, &b->upload, &b->pres_desc, &b->elem_seq_off, &b->pres_in, &b->pres_bits, &b->pres_out, &b->rows_sorted, &b->pos_query, &b->hsh, &b->rep, &b->seqs, &b->d_seq_off, &b->d_pos_off, &b->d_tab_off, &b->tab, &b->first_pos, &b->pos_unique, &b->tmp, &b->rows,
                      &b->num_kmers, &b->num_unique, &b->min_kmers, &b->bitmaps, &b->counts, &b->scratch, &b->excl_bits, &b->ranked, &b->win_col, &b->win_cnt, &b->win_loc})
        d->release();
    b->hits.release();
    b->ghits.release();
    b->gbuf.release();
    if (b->job.done) { e = hipEventSynchronize(b->job.done); e = hipEventDestroy(b->job.done); (void)e; }
    if (b->pin_up) { e = hipHostFree(b->pin_up); (void)e; }
    if (b->pin_out) { e = hipHostFree(b->pin_out); (void)e; }
    if (b->pin_flag) { e = hipHostFree(b->pin_flag); (void)e; }
    b->exp_count.release();
    if (b->job.h_in) { e = hipHostFree(b->job.h_in); (void)e; }
    if (b->job.h_out) { e = hipHostFree(b->job.h_out); (void)e; }
    if (b->done) { e = hipEventDestroy(b->done); (void)e; }
    if (b->g_done) { e = hipEventDestroy(b->g_done); (void)e; }
    delete b;
    return BIGSI_OK;
}

extern "C" int bigsi_hip_batch_set_result_cols(bigsi_hip_batch *b, uint64_t cols)
{
    BIGSI_ENTER(b ? b->ix : nullptr);
    if (!b) return fail(BIGSI_ERR_INVALID, "NULL batch");
    if (cols > b->ix->cap_cols)
        return fail(BIGSI_ERR_CAPACITY, "result width %llu exceeds col_capacity %llu (call bigsi_hip_reserve_cols)", (unsigned long long)cols,
                    (unsigned long long)b->ix->cap_cols);
    b->result_cols = cols;
    return BIGSI_OK;
}

extern "C" int bigsi_hip_batch_set_limit(bigsi_hip_batch *b, uint32_t limit, const uint32_t *excluded, uint64_t n_excluded)
{
    BIGSI_ENTER(b ? b->ix : nullptr);
    if (!b) return fail(BIGSI_ERR_INVALID, "NULL batch");
    if (n_excluded && !limit) return fail(BIGSI_ERR_INVALID, "excluded colours are only valid with a limit (limit = 0 is off)");
    if (n_excluded && !excluded) return fail(BIGSI_ERR_INVALID, "excluded is NULL");
    if (n_excluded > 0xFFFFFFFFull) return fail(BIGSI_ERR_INVALID, "too many excluded colours");
    if (limit == b->limit && b->excluded.size() == n_excluded && std::equal(b->excluded.begin(), b->excluded.end(), excluded)) return BIGSI_OK;
    b->limit = limit;
    b->excluded.assign(excluded, excluded + n_excluded);
    b->excl_words = 0;
    return BIGSI_OK;
}

extern "C" int bigsi_hip_batch_set_outputs(bigsi_hip_batch *b, void *d_bitmaps)
{
    BIGSI_ENTER(b ? b->ix : nullptr);
    if (!b) return fail(BIGSI_ERR_INVALID, "NULL batch");
    b->ext_bitmaps = d_bitmaps;
    return BIGSI_OK;
}

// -------- K2 dispatch
// what every launch of the counting kernel over a batch shares (the launches themselves: RowAndPlan::launch, bigsi_launch.hpp)
struct CountLaunch {
    const uint64_t *k2_rows;
    void *out;
    uint64_t out_stride;
    uint64_t *hit_bitmap;
    uint32_t sparse;
    bool deep;                  // software-pipelined row loads (small grids; h = 3 or 4 only)
    uint32_t early_exit;        // BIGSI_RUN_EARLY_EXIT on a hits-only, one-slice run
    uint64_t *partial;          // slices > 1: bit-sliced partial counts of every slice (k_count_combine adds them up)
    uint32_t planes_out;
};

// The counter planes `P` of a run -> the template instance <P, CountT> the counting kernels are compiled for: f(Planes<P, CountT>{})
template <int N, typename T>
struct Planes {
    static constexpr int P = N;
    using CountT = T;
};
template <typename F>
static void with_planes(int P, F &&f)
{
    switch (P) {
    case 6: f(Planes<6, uint16_t>{}); break;
    case 10: f(Planes<10, uint16_t>{}); break;
    case 12: f(Planes<12, uint16_t>{}); break;
    case 16: f(Planes<16, uint16_t>{}); break;
    default: f(Planes<32, uint32_t>{}); break;
    }
}

template <int P, typename CountT>
static void launch_count_wide(bigsi_hip_batch *b, const CountLaunch &c, const RowAndLaunch &l)
{
    bigsi_hip_index *ix = b->ix;
#define BIGSI_COUNT_ARGS                                                                                                      \
    dim3((unsigned)l.grid), dim3(l.block), 0, ix->stream, ix->d_index, ix->stride_words, (uint32_t)b->wv, c.k2_rows, b->d_pos_off.as<uint64_t>(), \
        b->num_unique.as<uint32_t>(), ix->h, l.q0, l.q1, l.tiles, (CountT *)c.out, c.out_stride, b->min_kmers.as<uint32_t>(), ix->n_cols,  \
        c.hit_bitmap, b->wv_pad, c.sparse, l.slices, c.early_exit, c.partial, c.planes_out
#define COMMA ,
#define BIGSI_LAUNCH_COUNT(H) hipLaunchKernelGGL((k_and_count<P, H, CountT>), BIGSI_COUNT_ARGS)
#define BIGSI_LAUNCH_COUNT_DEEP(H)                                                                        \
    if (c.deep) hipLaunchKernelGGL((k_and_count<P COMMA H COMMA CountT COMMA 2>), BIGSI_COUNT_ARGS);       \
    else hipLaunchKernelGGL((k_and_count<P, H, CountT>), BIGSI_COUNT_ARGS)
    switch (ix->h) {
    case 1: BIGSI_LAUNCH_COUNT(1); break;
    case 2: BIGSI_LAUNCH_COUNT(2); break;
    case 3: BIGSI_LAUNCH_COUNT_DEEP(3); break;
    case 4: BIGSI_LAUNCH_COUNT_DEEP(4); break;
    case 5: BIGSI_LAUNCH_COUNT(5); break;
    default: BIGSI_LAUNCH_COUNT(0); break;
    }
#undef BIGSI_LAUNCH_COUNT
#undef BIGSI_LAUNCH_COUNT_DEEP
#undef BIGSI_COUNT_ARGS
#undef COMMA
}

static void launch_count(bigsi_hip_batch *b, int P, const CountLaunch &c, const RowAndLaunch &l)
{
    with_planes(P, [&](auto pl) { launch_count_wide<decltype(pl)::P, typename decltype(pl)::CountT>(b, c, l); });
}

static int compact_local(bigsi_hip_batch *b, bool write_only);
static int rank_select(bigsi_hip_batch *b, const void *src, const void *counters, void *dst, hipStream_t st);

// Reads against a narrow index: K1 + K2 + K4 in one launch (k_reads_fused) when the batch qualifies.
static bool reads_fusable(const bigsi_hip_batch *b, uint32_t flags)
{
    const bigsi_hip_index *ix = b->ix;
    const bool exact = b->exact;
    return b->k == 31 && b->total_pos > 0 && b->max_pos <= 63 && b->n_seqs <= kReadsMaxSeqs && b->wv <= (uint64_t)kBlock * kVec &&
           ix->h >= 2 && ix->h <= 4 && !b->ext_bitmaps && b->result_cols == 0 && b->limit == 0 &&
           !(flags & (BIGSI_RUN_SKIP_COMPACT | BIGSI_RUN_K1_GLOBAL | BIGSI_RUN_EARLY_EXIT | BIGSI_RUN_NO_SORT | BIGSI_RUN_BAND_SWEEP)) &&
           (exact || (flags & BIGSI_RUN_SPARSE_COUNTS));     // the fused kernel keeps counters in registers: hits only
}

// Where K1 reads a load's tables and sequences.  Normally the device copies (create / reload / a flushed deferred load).  A one-call
// search whose input is small reads them straight from the pinned staging (zero copy: scripts/probe/latency_probe.hip prices a 64 KB
// hipMemcpyAsync ahead of a kernel at 23 us against 9.5 us of direct reads) and writes the device copy of pos_off -- all the later
// kernels need of them -- on its way.
struct K1Src {
    const char *seqs;
    const uint64_t *seq_off, *pos_off;
    uint64_t *pos_off_out;
    uint32_t one_len;          // > 0: the batch is one sequence of this length, read in place (no offset tables to fetch)
    // one_len > 0: the same bytes as the host sees them -- short enough, they travel in the kernel arguments instead (SeqArg)
    template <int N>
    SeqArg<N> by_value() const
    {
        SeqArg<N> a;
        memset(a.w, 0, sizeof a.w);
        memcpy(a.w, seqs, one_len);
        return a;
    }
};

static K1Src k1_src(const bigsi_hip_batch *b)
{
    if (b->zero_copy) {
        const uint8_t *h = static_cast<const uint8_t *>(b->pin_up);
        const size_t ob = (b->n_seqs + 1) * 8ull;
        return K1Src{reinterpret_cast<const char *>(h + 3 * ob), reinterpret_cast<const uint64_t *>(h), reinterpret_cast<const uint64_t *>(h + ob),
                     b->d_pos_off.as<uint64_t>(), b->n_seqs == 1 && b->max_len ? (uint32_t)b->max_len : 0u};
    }
    return K1Src{b->seqs.as<char>(), b->d_seq_off.as<uint64_t>(), b->d_pos_off.as<uint64_t>(), nullptr, 0u};
}

static int export_prepare(bigsi_hip_batch *b, hipStream_t st);

// `inline_export`: a one-call search of ONE read -- the kernel's only workgroup writes the caller's block and raises the flag itself
static int launch_reads_fused(bigsi_hip_batch *b, hipStream_t st = nullptr, bool inline_export = false)
{
    const uint32_t fp_mask = b->weak_fp ? 1u : ~0u;
    if (!st) st = b->ix->stream;
    bigsi_hip_index *ix = b->ix;
    HitBufs &hb = b->hits;
    TRY(b->bitmaps.reserve((size_t)b->n_seqs * b->wv_pad * 8));
    TRY(hb.hit_off.reserve((b->n_seqs + 2) * 8ull));          // (query-ordered offsets: filled by whoever orders the lists)
    if (hb.cap == 0 && !hb.xcol) {
        const uint64_t want = kHitsInitialCapacity;
        TRY(hb.hit_col.reserve(want * 4));
        TRY(hb.hit_cnt.reserve(want * 4));
        hb.cap = want;
    }
    // per query: where its hits start in the hit buffers and how many they are; two allocation counters used alternately (a
    // launch zeroes the one its successor will use: launches of one batch never overlap)
    TRY(hb.q_start.reserve((size_t)b->n_seqs * 8));
    TRY(hb.q_cnt.reserve((size_t)b->n_seqs * 4));
    if (!hb.alloc.p) {
        TRY(hb.alloc.reserve(256));
        HIP_TRY(hipMemsetAsync(hb.alloc.p, 0, 256, st));
        hb.gen = 0;
    }
    // (the generation advances only once the launch is queued: a launch that fails -- export_prepare, hipGetLastError -- leaves the
    // counters as the last successful launch left them, i.e. this slot still zeroed for the retry)
    const uint32_t gen_next = hb.gen + 1;
    b->exported_inline = false;
    if (inline_export) {
        TRY(export_prepare(b, st));
        b->exported_inline = true;
    }
    const K1Src src = k1_src(b);
    // one read read in place: its bytes go in the kernel arguments, not over the host link (SeqArg, bigsi_kernels.hpp)
    const bool by_arg = src.one_len && src.one_len <= kSeqArgRead;
    b->rpath.k1_parts = 1u;      // (bigsi_hip_batch_last_row_and: all a read run reports)
    b->rpath.k1_arg_bytes = by_arg ? kSeqArgRead : 0u;
    SeqArg<kSeqArgRead> read_arg;
    if (by_arg) read_arg = src.by_value<kSeqArgRead>();
    else memset(read_arg.w, 0, sizeof read_arg.w);
#define BIGSI_READS_ARGS                                                                                                          \
    dim3(b->n_seqs), dim3(kBlock), 0, st, ix->d_index, ix->stride_words, (uint32_t)b->wv, ix->n_cols, ix->m, b->threshold,              \
        by_arg ? (const char *)nullptr : src.seqs, src.seq_off, src.pos_off, b->n_seqs, b->first_pos.as<uint32_t>(),                        \
        b->pos_unique.as<uint32_t>(), b->rep.as<uint32_t>(), b->rows.as<uint64_t>(), b->num_kmers.as<uint32_t>(),                      \
        b->num_unique.as<uint32_t>(), b->min_kmers.as<uint32_t>(), b->bitmaps.as<uint64_t>(), b->wv_pad, hb.q_start.as<uint64_t>(),   \
        hb.q_cnt.as<uint32_t>(), hb.alloc.as<unsigned long long>(), gen_next & 1u, hb.col(), hb.cnt(), hb.capacity(), fp_mask,          \
        src.pos_off_out, src.one_len, b->exported_inline ? static_cast<uint64_t *>(b->pin_out) : nullptr, b->exp_spec,                          \
        (volatile uint64_t *)b->pin_flag, b->exp_serial, read_arg
#define COMMA ,
    // rows of at most kBlock words, counting: one word per lane (8-byte loads: half the registers -- 8 wavefronts per SIMD instead
    // of 4 -- and twice the lanes that hold columns).  Interleaved A/B at C2: counting 1377 -> 1523 M lookups/s; the exact kernel
    // (6 -> 8 wavefronts per SIMD) 1563 -> 1534 M: stays at two words per lane
    const bool narrow = b->wv <= (uint64_t)kBlock;
    // a handful of reads (a latency-bound call): the exact route splits each query's rows over the two halves of its workgroup
    const bool split = narrow && b->n_seqs <= 64;
#define BIGSI_READS(H)                                                                              \
    if (split && b->exact) hipLaunchKernelGGL((k_reads_fused<H COMMA true COMMA kVec COMMA 16 COMMA true>), BIGSI_READS_ARGS);     \
    else if (split) hipLaunchKernelGGL((k_reads_fused<H COMMA false COMMA kVec COMMA 16 COMMA true>), BIGSI_READS_ARGS);          \
    else if (b->exact) hipLaunchKernelGGL((k_reads_fused<H COMMA true>), BIGSI_READS_ARGS);                \
    else if (narrow) hipLaunchKernelGGL((k_reads_fused<H COMMA false COMMA 1>), BIGSI_READS_ARGS);       \
    else hipLaunchKernelGGL((k_reads_fused<H COMMA false>), BIGSI_READS_ARGS)
    switch (ix->h) {
    case 2: BIGSI_READS(2); break;
    case 3: BIGSI_READS(3); break;
    default: BIGSI_READS(4); break;
    }
#undef BIGSI_READS
#undef BIGSI_READS_ARGS
#undef COMMA
    HIP_TRY(hipGetLastError());
    hb.gen = gen_next;
    return BIGSI_OK;
}

// see bigsi_internal.hpp: the launch rule (bigsi_launch.hpp) for 256-thread workgroups
uint32_t bigsi_exact_launch_queries(const bigsi_hip_index *ix) { return exact_launch_queries(ceil_div(ix->n_cols, 64)); }

// the band sweep's plan for a run of n_seqs queries of at most max_pos positions on results of wv words (bigsi_batch_run; the stream
// sizes its exact chunks by it)
static BandSweepPlan band_plan(const bigsi_hip_index *ix, uint32_t n_seqs, uint64_t wv, uint64_t max_pos, bool exact, uint32_t flags)
{
    return plan_band_sweep(RowAndInput{n_seqs, wv, max_pos, ix->h, exact, (flags & BIGSI_RUN_NO_SORT) != 0, (flags & BIGSI_RUN_EARLY_EXIT) != 0,
                                       (flags & BIGSI_RUN_SPARSE_COUNTS) != 0},
                           ix->m, (flags & BIGSI_RUN_BAND_SWEEP) != 0, ix->band_windows, ix->band_segs);
}
bool bigsi_band_sweep_taken(const bigsi_hip_index *ix, uint32_t n_seqs, uint64_t max_pos, uint32_t flags)
{
    return !(flags & BIGSI_RUN_FORCE_COUNTS) && band_plan(ix, n_seqs, ceil_div(ix->n_cols, 64), max_pos, true, flags).taken;
}

static K1Plan k1_plan(const bigsi_hip_batch *b, bool force_global) { return k1_plan(b->n_seqs, b->max_pos, b->max_len, b->elements, force_global); }

// K1 for the whole batch (h may have changed since create: the rows buffer is sized for it here)
struct Preset {              // result words K1 sets for the sliced row-AND launches of a small batch (see k_kmerize_lds)
    uint64_t *p = nullptr;
    uint64_t words = 0, value = 0;
    bool done = false;       // the K1 route taken did it (the others leave it to a memset)
};

static int run_kmerize(bigsi_hip_batch *b, double threshold, const K1Plan &plan, bool want_sorted = false, bool *sorted = nullptr,
                       Preset *preset = nullptr)
{
    uint64_t *ps_p = preset ? preset->p : nullptr;
    const uint64_t ps_words = preset ? preset->words : 0, ps_value = preset ? preset->value : 0;
    bigsi_hip_index *ix = b->ix;
    EventPair ep{};
    hipStream_t ks = ix->stream;
    // K1 rewrites arrays a gathered compaction of the previous run of THIS batch may still be reading on the gather stream (on the
    // index stream itself the callers' own ordering applies, as for every other entry point)
    if (b->g_done && b->gstream && b->gstream != ks) HIP_TRY(hipStreamWaitEvent(ks, b->g_done, 0));
    TRY(b->rows.reserve(std::max<uint64_t>(b->total_pos, 1) * ix->h * 8));
    const K1Src src = k1_src(b);
    b->rpath.k1_parts = 1u;                // (bigsi_hip_batch_last_row_and; the LDS route says below what it took)
    b->rpath.k1_arg_bytes = 0u;
    if (plan.route == K1_ELEMENTS) {       // explicit k-mers: only the hashing is left of K1
        TRY(ev_begin(ix, &ep, ks));
        hipLaunchKernelGGL(k_rows_raw, dim3(b->n_seqs), dim3(kBlock), 0, ks, b->seqs.as<char>(), b->d_seq_off.as<uint64_t>(), b->elem_seq_off.as<uint64_t>(),
                           b->d_pos_off.as<uint64_t>(), ix->h, ix->m, threshold, b->rows.as<uint64_t>(), b->num_kmers.as<uint32_t>(),
                           b->num_unique.as<uint32_t>(), b->min_kmers.as<uint32_t>());
        HIP_TRY(hipGetLastError());
        TRY(ev_end(ix, &ep, ix->ev_km, ks));
        b->run_h = ix->h;
        return BIGSI_OK;
    }
    if (plan.route == K1_WAVE) {
        // probe / read-length queries: one wavefront per query, no LDS, no atomics
        TRY(ev_begin(ix, &ep, ks));
        const unsigned grid = (unsigned)ceil_div(b->n_seqs, kBlock / 64);
#define BIGSI_K1_WAVE(KF)                                                                                                      \
    hipLaunchKernelGGL((k_kmerize_wave<KF>), dim3(grid), dim3(kBlock), 0, ks, src.seqs, src.seq_off,                               \
                       src.pos_off, b->k, ix->h, ix->m, threshold, b->n_seqs, b->first_pos.as<uint32_t>(),                               \
                       b->pos_unique.as<uint32_t>(), b->rep.as<uint32_t>(), b->rows.as<uint64_t>(), b->num_kmers.as<uint32_t>(),           \
                       b->num_unique.as<uint32_t>(), b->min_kmers.as<uint32_t>(), ps_p, ps_words, ps_value, src.pos_off_out)
        if (b->k == 31) BIGSI_K1_WAVE(31);
        else BIGSI_K1_WAVE(0);
#undef BIGSI_K1_WAVE
        if (preset) preset->done = ps_p != nullptr;
        HIP_TRY(hipGetLastError());
        TRY(ev_end(ix, &ep, ix->ev_km, ks));
        b->run_h = ix->h;
        return BIGSI_OK;
    }
    const uint32_t hs_cap = plan.hs_cap, sq_bytes = plan.sq_bytes, tab_mult = plan.tab_mult, tab_cap = plan.tab_cap;
    const size_t lds = plan.lds;
    if (plan.route == K1_LDS) {
        // one thread per position for small batches (latency); once there are several queries per CU anyway, smaller
        // workgroups that loop over the positions let more queries overlap their barrier-separated phases
        const uint32_t block_cap = b->n_seqs >= 1024 ? 256u : 1024u;
        uint32_t block = 64;
        while (block < b->max_pos && block < block_cap) block <<= 1;
        if (want_sorted) {
            TRY(b->rows_sorted.reserve(std::max<uint64_t>(b->total_pos, 1) * ix->h * 8));
            if (sorted) *sorted = true;
        }
        TRY(ev_begin(ix, &ep, ks));
        // a handful of gene-length queries (a latency-bound call): the hashing of a query's unique k-mers is spread over several
        // workgroups (k_kmerize_lds, `parts`)
        const uint32_t parts = (!want_sorted && b->max_pos <= block && b->max_pos >= 256 && b->n_seqs <= 32) ? 8u : 1u;
#define BIGSI_K1_LDS_(KF, ARGB, SARG)                                                                                           \
    hipLaunchKernelGGL((k_kmerize_lds<KF, ARGB>), dim3(b->n_seqs * parts), dim3(block), lds, ks, src.seqs, src.seq_off,           \
                       src.pos_off, b->k, ix->h, ix->m, threshold, tab_cap, tab_mult, hs_cap, sq_bytes, b->first_pos.as<uint32_t>(), b->tmp.as<uint32_t>(), \
                       b->pos_unique.as<uint32_t>(), b->rep.as<uint32_t>(), b->rows.as<uint64_t>(), b->num_kmers.as<uint32_t>(),      \
                       b->num_unique.as<uint32_t>(), b->min_kmers.as<uint32_t>(), want_sorted ? b->rows_sorted.as<uint64_t>() : (uint64_t *)nullptr, \
                       ps_p, ps_words, ps_value, src.pos_off_out, src.one_len, parts, SARG)
        // one sequence read in place (a one-call search): short enough, its bytes go in the kernel arguments (SeqArg)
#define BIGSI_K1_LDS(KF)                                                                                   \
    if (src.one_len && src.one_len <= kSeqArgSmall) BIGSI_K1_LDS_(KF, kSeqArgSmall, src.by_value<kSeqArgSmall>());       \
    else if (src.one_len && src.one_len <= kSeqArgLarge) BIGSI_K1_LDS_(KF, kSeqArgLarge, src.by_value<kSeqArgLarge>());  \
    else BIGSI_K1_LDS_(KF, 0, SeqArg<0>{})
        if (b->k == 31) BIGSI_K1_LDS(31);
        else BIGSI_K1_LDS(0);
        b->rpath.k1_parts = parts;
        b->rpath.k1_arg_bytes = !src.one_len ? 0u : src.one_len <= kSeqArgSmall ? kSeqArgSmall : src.one_len <= kSeqArgLarge ? kSeqArgLarge : 0u;
#undef BIGSI_K1_LDS
#undef BIGSI_K1_LDS_
        if (preset) preset->done = ps_p != nullptr;
        HIP_TRY(hipGetLastError());
        TRY(ev_end(ix, &ep, ix->ev_km, ks));
        b->run_h = ix->h;
        return BIGSI_OK;
    }
    {   // the multi-launch route's scratch (allocated lazily: batches of short queries never need it)
        const uint64_t Tn = std::max<uint64_t>(b->total_pos, 1);
        TRY(b->tab.reserve(b->tab_off[b->n_seqs] * 4));
        TRY(b->hsh.reserve(Tn * 4));
        if (b->pos_query.cap < Tn * 4 || !b->pos_query_loaded) {
            TRY(b->pos_query.reserve(Tn * 4));
            std::vector<uint32_t> pq(b->total_pos);
            for (uint32_t i = 0; i < b->n_seqs; i++) std::fill(pq.begin() + b->pos_off[i], pq.begin() + b->pos_off[i + 1], i);
            if (b->total_pos) HIP_TRY(hipMemcpy(b->pos_query.p, pq.data(), b->total_pos * 4, hipMemcpyHostToDevice));
            b->pos_query_loaded = true;
        }
    }
    HIP_TRY(hipMemsetAsync(b->tab.p, 0xFF, b->tab_off[b->n_seqs] * 4, ks));
    TRY(ev_begin(ix, &ep, ks));
    const uint64_t T = b->total_pos;
    const unsigned pgrid = (unsigned)ceil_div(std::max<uint64_t>(T, 1), kBlock);
#define BIGSI_K1_INSERT(KF)                                                                                                   \
    hipLaunchKernelGGL((k_kmer_insert<KF>), dim3(pgrid), dim3(kBlock), 0, ks, b->seqs.as<char>(), b->d_seq_off.as<uint64_t>(), \
                       b->d_pos_off.as<uint64_t>(), b->pos_query.as<uint32_t>(), b->d_tab_off.as<uint64_t>(), b->tab.as<uint32_t>(), \
                       b->k, T, b->hsh.as<uint32_t>())
#define BIGSI_K1_ROWS(KF)                                                                                                     \
    hipLaunchKernelGGL((k_kmer_rows<KF>), dim3(pgrid), dim3(kBlock), 0, ks, b->seqs.as<char>(), b->d_seq_off.as<uint64_t>(), \
                       b->d_pos_off.as<uint64_t>(), b->pos_query.as<uint32_t>(), b->rep.as<uint32_t>(), b->tmp.as<uint32_t>(), b->k, \
                       ix->h, ix->m, T, b->rows.as<uint64_t>())
    if (T) {
        if (b->k == 31) BIGSI_K1_INSERT(31);
        else BIGSI_K1_INSERT(0);
        hipLaunchKernelGGL(k_kmer_resolve, dim3(pgrid), dim3(kBlock), 0, ks, b->seqs.as<char>(), b->d_seq_off.as<uint64_t>(),
                           b->d_pos_off.as<uint64_t>(), b->pos_query.as<uint32_t>(), b->d_tab_off.as<uint64_t>(), b->tab.as<uint32_t>(),
                           b->k, T, b->hsh.as<uint32_t>(), b->rep.as<uint32_t>());
    }
    hipLaunchKernelGGL(k_kmer_rank, dim3(b->n_seqs), dim3(kBlock), 0, ks, b->d_seq_off.as<uint64_t>(), b->d_pos_off.as<uint64_t>(),
                       b->rep.as<uint32_t>(), b->k, threshold, b->first_pos.as<uint32_t>(), b->tmp.as<uint32_t>(), b->pos_unique.as<uint32_t>(),
                       b->num_kmers.as<uint32_t>(), b->num_unique.as<uint32_t>(), b->min_kmers.as<uint32_t>());
    if (T) {
        if (b->k == 31) BIGSI_K1_ROWS(31);
        else BIGSI_K1_ROWS(0);
    }
#undef BIGSI_K1_INSERT
#undef BIGSI_K1_ROWS
    HIP_TRY(hipGetLastError());
    TRY(ev_end(ix, &ep, ix->ev_km, ks));
    b->run_h = ix->h;
    return BIGSI_OK;
}

// a deferred load (batch_load): the staged tables and sequences go up now, ahead of this run's first kernel on its stream
static int flush_upload(bigsi_hip_batch *b, hipStream_t st, bool k1_reads_host = false)
{
    if (!b->upload_deferred) return BIGSI_OK;
    // a one-call search with a small input: this run's K1 (one of the single-launch routes) reads pin_up itself
    b->zero_copy = k1_reads_host && b->one_call && b->pin_up_bytes <= kZeroCopyBytes;
    // ... unless many workgroups would each fetch their own few bytes over the link: then one small kernel copies the staging
    // with wide loads first (k_stage_in), and K1 reads the device arrays
    if (b->zero_copy && b->n_seqs > 1 && b->pin_up_bytes >= (size_t)(8 << 10)) {
        const unsigned grid = (unsigned)std::min<uint64_t>(ceil_div(b->pin_up_bytes, (uint64_t)kBlock * 16), 64);
        hipLaunchKernelGGL(k_stage_in, dim3(grid), dim3(kBlock), 0, st, static_cast<const uint8_t *>(b->pin_up), b->upload.as<uint8_t>(), (uint64_t)b->pin_up_bytes);
        HIP_TRY(hipGetLastError());
        b->zero_copy = false;
    } else if (!b->zero_copy) HIP_TRY(hipMemcpyAsync(b->upload.p, b->pin_up, b->pin_up_bytes, hipMemcpyHostToDevice, st));
    b->upload_deferred = false;
    return BIGSI_OK;
}

// This batch's own earlier work that the run about to be queued on `st` must not overtake: K1 rewrites arrays it may still be
// reading.  A batch that `was_idle` (nothing of it in flight: collected since its last run) has no waits to queue.
// `gather`: a gathered compaction on the gather stream too -- a run whose K1 is run_kmerize leaves that wait to it.
static int wait_previous(bigsi_hip_batch *b, hipStream_t st, bool was_idle, bool gather)
{
    if (was_idle) return BIGSI_OK;
    // its previous run (one-call runs record no event: bigsi_batch_run)
    if (b->done_stale && b->run_stream && b->run_stream != st) HIP_TRY(hipStreamSynchronize(b->run_stream));
    else if (b->done && b->run_stream != st) HIP_TRY(hipStreamWaitEvent(st, b->done, 0));
    if (gather && b->g_done && b->gstream && b->gstream != st) HIP_TRY(hipStreamWaitEvent(st, b->g_done, 0));
    // a K5 / K6 request of this batch still in flight on another stream reads what K1 is about to rewrite
    if (b->job.done && b->job.device_work) HIP_TRY(hipStreamWaitEvent(st, b->job.done, 0));
    return BIGSI_OK;
}

// End of a run whose last kernel went out on `st`: the completion event (not for a one-call run: bigsi_batch_run) and, on the
// index stream, what later read-kernel launches wait for.
static int finish_run(bigsi_hip_batch *b, hipStream_t st, bool one_call, bool index_stream)
{
    b->done_stale = one_call;
    if (!one_call) {
        if (!b->done) HIP_TRY(hipEventCreateWithFlags(&b->done, hipEventDisableTiming));
        HIP_TRY(hipEventRecord(b->done, st));
    }
    if (index_stream) TRY(mark_main(b->ix));
    b->run_stream = st;
    b->ran = true;
    b->dirty = false;
    return BIGSI_OK;
}

// `one_call`: the caller is bigsi_hip_search_batch, which waits for this run through the export's flag on the same stream: the
// completion event is not recorded (one HIP call less on a path whose device work is a few microseconds); everything that would
// wait for it waits for the stream instead (done_stale).
int bigsi_batch_run(bigsi_hip_batch *b, double threshold, uint32_t flags, bool one_call)
{
    if (!b) return fail(BIGSI_ERR_INVALID, "NULL batch");
    if (!(threshold <= 1.0)) return fail(BIGSI_ERR_INVALID, "threshold must be <= 1 (bigsi/graph/bigsi.py:176), got %g", threshold);
    bigsi_hip_index *ix = b->ix;
    // (a shard of a wider index may be empty: its result vectors, result_cols wide, are then all zero)
    if (ix->n_cols == 0 && b->result_cols == 0) return fail(BIGSI_ERR_STATE, "index has no columns");
    TRY(use_device(ix));
    const bool was_idle = b->idle;
    b->idle = false;
    b->ran = false;
    b->host_counts_valid = false;
    b->run_serial++;
    b->threshold = threshold;
    b->exact = (threshold == 1.0) && !(flags & BIGSI_RUN_FORCE_COUNTS);
    // result vectors as wide as the index, or as the shard width agreed by a group of column shards (uneven shards then
    // still exchange buffers of one geometry; words beyond this shard's num_cols are zero through valid_mask)
    b->wv = ceil_div(std::max(ix->n_cols, b->result_cols), 64);
    if (b->wv > ix->stride_words)
        return fail(BIGSI_ERR_CAPACITY, "result width %llu columns exceeds the row stride (call bigsi_hip_reserve_cols)", (unsigned long long)b->result_cols);
    b->wv_pad = round_up(b->wv, 2);

    b->fused_run = false;
    b->exported_inline = false;
    b->path = bigsi_hip_hits_path{};
    b->rpath = bigsi_hip_row_and_path{};
    if (reads_fusable(b, flags)) {
        // (K1 rewrites arrays the previous run of this batch may still be reading, on a read stream or the gather stream)
        TRY(b->rows.reserve(std::max<uint64_t>(b->total_pos, 1) * ix->h * 8));
        EventPair fe{};
        b->dirty = true;
        hipStream_t st = ix->stream;
        if (!(flags & BIGSI_RUN_ONE_STREAM)) TRY(read_stream(ix, &st));
        else if (ix->rd_pending) TRY(quiesce_reads(ix));      // (alone on the device: nothing of the read streams beside it)
        // (the compaction kernel of a gene-length batch waits between workgroups too: such a run is over before read kernels start)
        if (ix->main_ev && st != ix->stream) HIP_TRY(hipStreamWaitEvent(st, ix->main_ev, 0));
        TRY(wait_previous(b, st, was_idle, true));
        TRY(flush_upload(b, st, true));
        TRY(ev_begin(ix, &fe, st, true));
        b->weak_fp = (flags & BIGSI_RUN_WEAK_FINGERPRINT) != 0;
        TRY(launch_reads_fused(b, st, one_call && b->n_seqs == 1));
        TRY(ev_end(ix, &fe, ix->ev_and, st));
        b->run_h = ix->h;
        b->fused_run = true;
        b->path.one_launch = 1;
        b->path.inline_export = b->exported_inline ? 1 : 0;
        b->count_bytes = 2;
        b->sparse_counts = !b->exact;
        b->compacted = true;
        return finish_run(b, st, one_call, false);
    }

    // read kernels of other batches still in flight on the read streams: over before this run's kernels start (its hit
    // compaction waits between workgroups, as they do; each kind has the device to its own launches)
    TRY(quiesce_reads(ix));
    // (with them an earlier run of this batch on a read stream: whatever it ran on last, only its K5 / K6 request is left to wait for)
    b->run_stream = ix->stream;
    TRY(wait_previous(b, ix->stream, was_idle, false));

    // the plans: K1's route and the row-AND launches (bigsi_launch.hpp)
    const K1Plan k1 = k1_plan(b, (flags & BIGSI_RUN_K1_GLOBAL) != 0);
    const RowAndPlan plan = plan_row_and(RowAndInput{b->n_seqs, b->wv, b->max_pos, ix->h, b->exact, (flags & BIGSI_RUN_NO_SORT) != 0,
                                                     (flags & BIGSI_RUN_EARLY_EXIT) != 0, (flags & BIGSI_RUN_SPARSE_COUNTS) != 0});
    // a large exact batch whose queries share rows: one band of every query per launch instead (plan_band_sweep)
    const BandSweepPlan band = band_plan(ix, b->n_seqs, b->wv, b->max_pos, b->exact, flags);
    // (several windows: the bounds are cut at k_sort_rows' buckets, the same for every query; K1's own sort has a shift per query)
    const bool band_sorts = band.taken && band.windows > 1;
    // the sliced launches combine into preset result words (all ones for the AND, zero counters): K1 sets them on its way
    Preset preset;
    if (plan.preset) {
        if (!b->ext_bitmaps) TRY(b->bitmaps.reserve((size_t)b->n_seqs * b->wv_pad * 8));
        preset.p = (uint64_t *)b->bit_vectors(); preset.words = b->wv_pad; preset.value = ~0ull;
    }
    // K1 (its LDS route emits the sorted list itself; the other routes leave that to k_sort_rows below)
    EventPair ep{};
    bool sorted_by_k1 = false;
    TRY(flush_upload(b, ix->stream, k1.route == K1_WAVE || k1.route == K1_LDS));
    TRY(run_kmerize(b, threshold, k1, (plan.want_sorted || band.taken) && !band_sorts, &sorted_by_k1, &preset));
    b->dirty = true;        // until finish_run
    const uint64_t *k2_rows = sorted_by_k1 ? b->rows_sorted.as<uint64_t>() : b->rows.as<uint64_t>();
    const uint32_t shift = sort_shift(ix->m, kSortBuckets);
    const uint32_t sort_block = sort_rows_block(b->max_pos, ix->h);
    {   // (bigsi_hip_batch_last_row_and: a few host fields per run)
        bigsi_hip_row_and_path &rp = b->rpath;
        rp.k1_route = (uint32_t)k1.route;
        rp.band_taken = band.taken ? 1u : 0u;
        rp.band_windows = band.taken ? band.windows : 0u;
        rp.band_launches = band.taken ? band.n_launches : 0u;
        rp.slices = plan.slices; rp.block = plan.block; rp.tiles = plan.tiles; rp.chunk_q = plan.chunk_q; rp.n_launches = plan.n_launches;
        if (plan.n_launches) {
            const RowAndLaunch l = plan.launch(plan.n_launches - 1);
            rp.last_slices = l.slices; rp.last_block = l.block; rp.last_unroll = l.unroll;
        }
        const bool sorts = (plan.want_sorted || band.taken) && !sorted_by_k1;
        rp.sorted_by = sorted_by_k1 ? BIGSI_SORTED_BY_K1 : !sorts ? BIGSI_SORTED_BY_NONE : sort_block == 1024 ? BIGSI_SORTED_BY_SORT1024 : BIGSI_SORTED_BY_SORT256;
        rp.early_exit = (b->exact && !band.taken && (flags & BIGSI_RUN_EARLY_EXIT)) ? 1u : (!b->exact && plan.early) ? 1u : 0u;
        rp.preset_by = !plan.preset ? 0u : preset.done ? 1u : 2u;
        rp.zero_copy = b->zero_copy ? 1u : 0u;
        b->sorted_tab_mult = k1.tab_mult;
    }
    if ((plan.want_sorted || band.taken) && !sorted_by_k1) {
        TRY(b->rows_sorted.reserve(std::max<uint64_t>(b->total_pos, 1) * ix->h * 8));
        TRY(ev_begin(ix, &ep));
        // 1024 threads per query for long row lists (a 1 kbp query at h=4 has 3880 rows), 256 otherwise
        if (sort_block == 1024)
            hipLaunchKernelGGL((k_sort_rows<1024>), dim3(b->n_seqs), dim3(1024), 0, ix->stream, b->rows.as<uint64_t>(), b->rows_sorted.as<uint64_t>(),
                               b->d_pos_off.as<uint64_t>(), b->num_unique.as<uint32_t>(), ix->h, 1u, shift);
        else
            hipLaunchKernelGGL((k_sort_rows<kBlock>), dim3(b->n_seqs), dim3(kBlock), 0, ix->stream, b->rows.as<uint64_t>(), b->rows_sorted.as<uint64_t>(),
                               b->d_pos_off.as<uint64_t>(), b->num_unique.as<uint32_t>(), ix->h, 1u, shift);
        HIP_TRY(hipGetLastError());
        TRY(ev_end(ix, &ep, ix->ev_km));
        k2_rows = b->rows_sorted.as<uint64_t>();
    }
    // K2: the plan's launches
    if (plan.too_large) return fail(BIGSI_ERR_INVALID, "batch too large for one launch (%llu workgroups)", (unsigned long long)plan.too_large);
    if (b->exact) {
        if (!b->ext_bitmaps) TRY(b->bitmaps.reserve((size_t)b->n_seqs * b->wv_pad * 8));
        uint64_t *out = (uint64_t *)b->bit_vectors();
        if (plan.preset && !preset.done) HIP_TRY(hipMemsetAsync(out, 0xFF, (size_t)b->n_seqs * b->wv_pad * 8, ix->stream));
        TRY(ev_begin(ix, &ep, nullptr, true));
        for (uint32_t i = 0; i < band.n_launches; i++) {
            const BandLaunch l = band.launch(i);
            const BandWindow w = band_window(ix->m, l.window, band.windows, shift);
            hipLaunchKernelGGL((k_and_exact_band<kBandUnroll, false>), dim3((unsigned)l.grid), dim3(kBlock), 0, ix->stream, ix->d_index, ix->stride_words,
                               (uint32_t)b->wv, ix->n_cols, k2_rows, b->d_pos_off.as<uint64_t>(), b->num_unique.as<uint32_t>(), ix->h, b->n_seqs, l.seg0,
                               l.nseg, w.lo, w.hi, l.window == 0 ? 1u : 0u, l.window + 1 == band.windows ? 1u : 0u, out, b->wv_pad);
        }
        for (uint32_t i = 0; i < (band.taken ? 0u : plan.n_launches); i++) {
            const RowAndLaunch l = plan.launch(i);
            // (a sliced last launch of an unsliced batch: its words alone)
            if (l.needs_preset && !plan.preset)
                HIP_TRY(hipMemsetAsync(out + (uint64_t)l.q0 * b->wv_pad, 0xFF, (size_t)(l.q1 - l.q0) * b->wv_pad * 8, ix->stream));
#define BIGSI_LAUNCH_EXACT(U)                                                                                                  \
    hipLaunchKernelGGL((k_and_exact<U>), dim3((unsigned)l.grid), dim3(l.block), 0, ix->stream, ix->d_index, ix->stride_words, (uint32_t)b->wv, \
                       ix->n_cols, k2_rows, b->d_pos_off.as<uint64_t>(), b->num_unique.as<uint32_t>(), ix->h, l.q0,    \
                       l.q1, l.tiles, out, b->wv_pad, l.slices, (flags & BIGSI_RUN_EARLY_EXIT) ? 1u : 0u)
            if (l.unroll == 4) BIGSI_LAUNCH_EXACT(4);
            else BIGSI_LAUNCH_EXACT(8);
#undef BIGSI_LAUNCH_EXACT
        }
        HIP_TRY(hipGetLastError());
        TRY(ev_end(ix, &ep, ix->ev_and, nullptr, band.taken ? band.n_launches : plan.n_launches));
    } else {
        b->count_bytes = plan.count_bytes;
        const uint64_t cstride = b->wv_pad * 64;
        TRY(b->counts.reserve((size_t)b->n_seqs * cstride * b->count_bytes));
        void *out = b->counters();
        // the kernel also leaves the thresholded hit bitmap (count >= min_kmers), which is what K4 compacts on a single GPU
        TRY(b->bitmaps.reserve((size_t)b->n_seqs * b->wv_pad * 8));
        uint64_t *hb = (uint64_t *)b->bit_vectors();
        b->sparse_counts = (flags & BIGSI_RUN_SPARSE_COUNTS) != 0;
        const uint32_t sparse = b->sparse_counts ? 1u : 0u;
        // a sliced (small) batch: every slice leaves its partial counts bit-sliced in scratch memory and k_count_combine adds them up
        uint64_t *partial = nullptr;
        if (plan.combine) {
            TRY(b->planes.reserve((size_t)b->n_seqs * plan.slices * plan.planes_out * b->wv_pad * 8));
            partial = b->planes.as<uint64_t>();
        }
        TRY(ev_begin(ix, &ep, nullptr, true));
        const CountLaunch cl{k2_rows, out, cstride, hb, sparse, plan.deep, plan.early ? 1u : 0u, partial, plan.planes_out};
        for (uint32_t i = 0; i < plan.n_launches; i++) launch_count(b, plan.P, cl, plan.launch(i));
        if (plan.combine) {        // the slices' partial counts -> totals, hit mask, counters
            with_planes(plan.P, [&](auto pl) {
                using CountT = typename decltype(pl)::CountT;
                hipLaunchKernelGGL((k_count_combine<decltype(pl)::P, CountT>), dim3((unsigned)plan.combine_grid), dim3(kBlock), 0, ix->stream, partial, plan.slices,
                                   plan.planes_out, b->wv_pad, (uint32_t)b->wv, b->n_seqs, b->num_unique.as<uint32_t>(), b->min_kmers.as<uint32_t>(),
                                   ix->n_cols, hb, (CountT *)out, cstride, sparse);
            });
        }
        HIP_TRY(hipGetLastError());
        TRY(ev_end(ix, &ep, ix->ev_and, nullptr, plan.n_launches));
    }

    b->compacted = !(flags & BIGSI_RUN_SKIP_COMPACT);
    if (!b->compacted) {
        // a member of a device group: its slot of the gather buffer goes into the exchange already trimmed to this shard's top N
        if (b->limit && b->ext_bitmaps) {
            TRY(ev_begin(ix, &ep));
            TRY(rank_select(b, b->ext_bitmaps, b->exact ? nullptr : b->counters(), b->ext_bitmaps, ix->stream));
            TRY(ev_end(ix, &ep, ix->ev_cp));
        }
        return finish_run(b, ix->stream, false, true);      // (the group waits for the event, whoever started the run)
    }
    // K4 on this shard's own result
    TRY(ev_begin(ix, &ep));
    TRY(compact_local(b, false));
    TRY(ev_end(ix, &ep, ix->ev_cp));
    return finish_run(b, ix->stream, one_call, true);
}

extern "C" int bigsi_hip_batch_run(bigsi_hip_batch *b, double threshold, uint32_t flags)
{
    BIGSI_ENTER(b ? b->ix : nullptr);
    return bigsi_batch_run(b, threshold, flags, false);
}

// The one launch of k_rank_select (rank_select below; bigsi_hip_rank_select_arrays): one workgroup per query over n_seqs x stride_words
// hit words, of which the first wv are the result; counters n_seqs x 64 * stride_words of count_bytes each (2: uint16_t, 4: uint32_t),
// null on an exact run, which takes the uint16_t instance and reads neither them nor num_unique / min_kmers.
static void launch_rank_select(uint32_t n_seqs, const uint64_t *src, uint64_t stride_words, uint32_t wv, const void *counters, uint32_t count_bytes,
                               const uint32_t *num_unique, const uint32_t *min_kmers, const uint64_t *excluded, uint32_t limit, uint64_t *dst,
                               hipStream_t st)
{
    if (count_bytes == 4 && counters)
        hipLaunchKernelGGL((k_rank_select<uint32_t>), dim3(n_seqs), dim3(kBlock), 0, st, src, stride_words, wv, (const uint32_t *)counters,
                           stride_words * 64, num_unique, min_kmers, excluded, limit, dst);
    else
        hipLaunchKernelGGL((k_rank_select<uint16_t>), dim3(n_seqs), dim3(kBlock), 0, st, src, stride_words, wv, (const uint16_t *)counters,
                           stride_words * 64, num_unique, min_kmers, excluded, limit, dst);
}

// k_rank_select over the batch's hit vectors `src` (counters: the counting run's, null on the exact path) into `dst` (may be `src`),
// n_seqs x wv_pad words.  The excluded colours' bit vector is built on first use and again whenever the result width outgrew it.
static int rank_select(bigsi_hip_batch *b, const void *src, const void *counters, void *dst, hipStream_t st)
{
    const uint64_t *ex = nullptr;
    if (!b->excluded.empty()) {
        if (b->excl_words < b->wv) {
            std::vector<uint64_t> words(b->wv_pad, 0ull);
            for (uint32_t c : b->excluded)
                if (c < b->wv_pad * 64) words[c / 64] |= 1ull << bit_of_col(c % 64);
            HIP_TRY(hipStreamSynchronize(st));      // (an earlier run of this batch may still read the old vector)
            TRY(b->excl_bits.reserve(b->wv_pad * 8));
            HIP_TRY(hipMemcpy(b->excl_bits.p, words.data(), b->wv_pad * 8, hipMemcpyHostToDevice));
            b->excl_words = b->wv_pad;
        }
        ex = b->excl_bits.as<uint64_t>();
    }
    if (b->n_seqs == 0) return BIGSI_OK;
    launch_rank_select(b->n_seqs, (const uint64_t *)src, b->wv_pad, (uint32_t)b->wv, counters, b->count_bytes, b->num_unique.as<uint32_t>(),
                       b->min_kmers.as<uint32_t>(), ex, b->limit, (uint64_t *)dst, st);
    HIP_TRY(hipGetLastError());
    return BIGSI_OK;
}

// K4 over the bit vectors `src`, [n_shards][seq][wv_pad] words (the exact AND, or the counting kernel's fused count >= min_kmers
// mask): group totals, then prefix + ordered write (k_hits_totals, k_hits_write: no waiting between workgroups).  A hit's count
// comes from `counters` (null on the exact path: every hit has count == num_unique), which hold shard `own_shard` alone or, with
// kAllShards, every shard.  `write_only` (the lists overflowed and were grown) runs the write pass again: the totals are still there.
static int compact_bits(bigsi_hip_batch *b, HitBufs &hb, const void *src, const void *counters, uint32_t n_shards, uint64_t shard_cols,
                        bool write_only, hipStream_t st, uint32_t own_shard)
{
    const uint32_t chunks = (uint32_t)ceil_div(b->wv, kBlock);
    const uint64_t nchunks = (uint64_t)n_shards * chunks * b->n_seqs;
    if (nchunks > 0x7FFFFFFFull) return fail(BIGSI_ERR_INVALID, "too many compaction chunks");
    TRY(hb.hit_off.reserve((b->n_seqs + 1) * 8ull));
    if (hb.cap == 0 && !hb.xcol) {
        const uint64_t want = kHitsInitialCapacity;
        TRY(hb.hit_col.reserve(want * 4));
        TRY(hb.hit_cnt.reserve(want * 4));
        hb.cap = want;
    }
    // a handful of items (one or two gene-length queries: a latency-bound call) go to ONE workgroup, which needs nobody's totals
    const HitsPlan hp = plan_hits(nchunks, n_shards);
    const uint32_t ipb = hp.ipb;
    const uint64_t ngroups = hp.groups;
    TRY(hb.chunk_hits.reserve(kHitsMaxGroups * 4));
    if (!write_only && ngroups > 1)
        hipLaunchKernelGGL(k_hits_totals, dim3((unsigned)ngroups), dim3(kBlock), 0, st, (const uint64_t *)src, b->wv_pad, (uint32_t)b->wv, b->n_seqs,
                           n_shards, chunks, ipb, hb.chunk_hits.as<uint32_t>());
    // a one-call search whose compaction is ONE workgroup (a gene-length query or two): that workgroup exports the results itself
    const bool inline_export = b->one_call && &hb == &b->hits && !write_only && hp.single && st == b->ix->stream;
    if (inline_export) {
        TRY(export_prepare(b, st));
        b->exported_inline = true;
    }
    // (bigsi_hip_hits_last_path)
    b->path.groups = (uint32_t)ngroups;
    b->path.items_per_group = ipb;
    b->path.single_workgroup = hp.single ? 1 : 0;
    if (write_only) b->path.rewrites++;
    else b->path.inline_export = inline_export ? 1 : 0;
    hipLaunchKernelGGL(k_hits_write, dim3((unsigned)ngroups), dim3(kBlock), 0, st, (const uint64_t *)src, b->wv_pad, (uint32_t)b->wv, b->n_seqs,
                       n_shards, chunks, shard_cols, b->num_unique.as<uint32_t>(), ipb, hb.chunk_hits.as<uint32_t>(),
                       hb.hit_off.as<uint64_t>(), hb.col(), hb.cnt(), hb.capacity(), counters, b->count_bytes, b->wv_pad * 64, own_shard,
                       inline_export ? static_cast<uint64_t *>(b->pin_out) : nullptr, b->exp_spec, b->uniq.as<uint32_t>(),
                       (volatile uint64_t *)b->pin_flag, b->exp_serial);
    HIP_TRY(hipGetLastError());
    return BIGSI_OK;
}

// K4 on this shard's own result vectors, into b->hits
static int compact_local(bigsi_hip_batch *b, bool write_only)
{
    const void *bm = b->bit_vectors(), *counters = b->exact ? nullptr : b->counters();
    if (b->limit) {
        // a result limit: K4 compacts the trimmed copy; the untrimmed vectors stay for fetch_bitmap / fetch_counts
        if (!write_only) {
            TRY(b->ranked.reserve((size_t)b->n_seqs * b->wv_pad * 8));
            TRY(rank_select(b, bm, counters, b->ranked.p, b->ix->stream));
        }
        bm = b->ranked.p;
    }
    return compact_bits(b, b->hits, bm, counters, 1, b->ix->n_cols, write_only, b->ix->stream, kAllShards);
}

// K4 on the bit vectors gathered from all shards (b->g_*), into b->ghits, on the gather stream
static int compact_gathered(bigsi_hip_batch *b, bool write_only)
{
    return compact_bits(b, b->ghits, b->g_src, b->exact ? nullptr : b->counters(), b->g_shards, b->g_shard_cols, write_only,
                        b->gstream ? b->gstream : b->ix->stream, b->g_own);
}

// A one-launch read run leaves every query's hits where its workgroup allocated them (k_reads_fused: no order between queries).
// fetch_hits brings them to the host in QUERY order: the totals decide whether the lists fit (grow + launch again if not), the
// per-query (start, count) pairs give the offsets, one download of the used part of the buffers and one pass over the queries
// put every list at its place.  The batch's `done` event has been waited for.
static int fetch_read_hits(bigsi_hip_batch *b, uint64_t *hit_offsets, uint32_t *colours, uint32_t *counts, uint64_t capacity)
{
    HitBufs &hb = b->hits;
    hipStream_t st = b->run_stream ? b->run_stream : b->ix->stream;
    const uint32_t n = b->n_seqs;
    unsigned long long total = 0;
    for (int attempt = 0;; attempt++) {
        HIP_TRY(hipMemcpy(&total, hb.alloc.as<unsigned long long>() + (hb.gen & 1u), 8, hipMemcpyDeviceToHost));
        if (total <= hb.capacity()) break;
        if (hb.xcol) {
            if (hit_offsets) memset(hit_offsets, 0, (n + 1) * 8ull), hit_offsets[n] = total;
            return fail(BIGSI_ERR_CAPACITY, "caller-owned hit buffers hold %llu entries, %llu needed", (unsigned long long)hb.xcap, total);
        }
        if (attempt) return fail(BIGSI_ERR_HIP, "internal: a read run overflowed hit buffers sized for its own total");
        TRY(hb.hit_col.reserve(total * 4));          // counters lived in registers: the whole pass again, on the stream it ran on
        TRY(hb.hit_cnt.reserve(total * 4));
        hb.cap = total;
        b->path.rewrites++;
        TRY(launch_reads_fused(b, st));
        HIP_TRY(hipStreamSynchronize(st));
    }
    std::vector<uint32_t> qc(n);
    std::vector<uint64_t> off(n + 1), qs;
    HIP_TRY(hipMemcpy(qc.data(), hb.q_cnt.p, n * 4ull, hipMemcpyDeviceToHost));
    off[0] = 0;
    for (uint32_t q = 0; q < n; q++) off[q + 1] = off[q] + qc[q];
    if (off[n] != total) return fail(BIGSI_ERR_HIP, "internal: hit counts of a read run do not add up (%llu vs %llu)", (unsigned long long)off[n], total);
    if (hit_offsets) memcpy(hit_offsets, off.data(), (n + 1) * 8ull);
    if (total > capacity)
        return fail(BIGSI_ERR_CAPACITY, "hit buffers hold %llu entries, %llu needed", (unsigned long long)capacity, total);
    if (!total || (!colours && !counts)) return BIGSI_OK;
    qs.resize(n);
    HIP_TRY(hipMemcpy(qs.data(), hb.q_start.p, n * 8ull, hipMemcpyDeviceToHost));
    std::vector<uint32_t> ucol(colours ? total : 0), ucnt(counts ? total : 0);
    if (colours) HIP_TRY(hipMemcpy(ucol.data(), hb.col(), total * 4, hipMemcpyDeviceToHost));
    if (counts) HIP_TRY(hipMemcpy(ucnt.data(), hb.cnt(), total * 4, hipMemcpyDeviceToHost));
    for (uint32_t q = 0; q < n; q++) {
        if (!qc[q]) continue;
        if (colours) memcpy(colours + off[q], ucol.data() + qs[q], qc[q] * 4ull);
        if (counts) memcpy(counts + off[q], ucnt.data() + qs[q], qc[q] * 4ull);
    }
    return BIGSI_OK;
}

// synchronise, make sure the hit lists fit (grow + rewrite if the write pass overflowed), copy them out
static int fetch_hits_from(bigsi_hip_batch *b, bool gathered, uint64_t *hit_offsets, uint32_t *colours, uint32_t *counts, uint64_t capacity)
{
    if (!gathered && b->fused_run) return fetch_read_hits(b, hit_offsets, colours, counts, capacity);
    HitBufs &hb = gathered ? b->ghits : b->hits;
    hipStream_t st = (gathered && b->gstream) ? b->gstream : b->ix->stream;
    std::vector<uint64_t> off(b->n_seqs + 2);
    // local hit lists were produced before b->done (already waited for); gathered ones on the gather stream
    if (gathered || !b->compacted) HIP_TRY(hipStreamSynchronize(st));
    HIP_TRY(hipMemcpy(off.data(), hb.hit_off.p, (b->n_seqs + 1) * 8ull, hipMemcpyDeviceToHost));
    const uint64_t total = off[b->n_seqs];
    if (hb.xcol && total > hb.xcap) {
        if (hit_offsets) memcpy(hit_offsets, off.data(), (b->n_seqs + 1) * 8ull);
        return fail(BIGSI_ERR_CAPACITY, "caller-owned hit buffers hold %llu entries, %llu needed", (unsigned long long)hb.xcap, (unsigned long long)total);
    }
    if (!hb.xcol && total > hb.cap) {
        TRY(hb.hit_col.reserve(total * 4));
        TRY(hb.hit_cnt.reserve(total * 4));
        hb.cap = total;
        TRY(gathered ? compact_gathered(b, true) : compact_local(b, true));
        if (gathered && b->comm && !b->exact) TRY(bigsi_reduce_gathered_counts(b));   // every rank takes this branch: totals are identical
        HIP_TRY(hipStreamSynchronize(st));
    }
    if (hit_offsets) memcpy(hit_offsets, off.data(), (b->n_seqs + 1) * 8ull);
    if (total > capacity)
        return fail(BIGSI_ERR_CAPACITY, "hit buffers hold %llu entries, %llu needed", (unsigned long long)capacity, (unsigned long long)total);
    if (total && colours) HIP_TRY(hipMemcpy(colours, hb.col(), total * 4, hipMemcpyDeviceToHost));
    if (total && counts) HIP_TRY(hipMemcpy(counts, hb.cnt(), total * 4, hipMemcpyDeviceToHost));
    return BIGSI_OK;
}

static int need_run(bigsi_hip_batch *b)
{
    if (!b) return fail(BIGSI_ERR_INVALID, "NULL batch");
    if (!b->ran) return fail(BIGSI_ERR_STATE, "bigsi_hip_batch_run has not completed for this batch");
    TRY(use_device(b->ix));
    if (b->idle) return BIGSI_OK;
    if (b->done_stale && b->run_stream) HIP_TRY(hipStreamSynchronize(b->run_stream));
    else if (b->done) HIP_TRY(hipEventSynchronize(b->done));      // this batch's kernels; later batches may still be running
    return BIGSI_OK;
}

static int host_counts(bigsi_hip_batch *b)
{
    if (b->host_counts_valid) return BIGSI_OK;
    const size_t n = b->n_seqs;
    b->h_uniq.resize(3 * n);
    HIP_TRY(hipMemcpy(b->h_uniq.data(), b->uniq.p, 3 * n * 4, hipMemcpyDeviceToHost));       // (point_uniq)
    b->h_num_kmers.assign(b->h_uniq.begin(), b->h_uniq.begin() + n);
    b->h_num_unique.assign(b->h_uniq.begin() + n, b->h_uniq.begin() + 2 * n);
    b->h_min_kmers.assign(b->h_uniq.begin() + 2 * n, b->h_uniq.end());
    b->host_counts_valid = true;
    return BIGSI_OK;
}

extern "C" int bigsi_hip_batch_get_info(bigsi_hip_batch *b, bigsi_hip_batch_info *out)
{
    BIGSI_ENTER(b ? b->ix : nullptr);
    if (!b || !out) return fail(BIGSI_ERR_INVALID, "NULL argument");
    memset(out, 0, sizeof *out);
    out->n_seqs = b->n_seqs;
    out->k = b->k;
    out->total_kmers = b->total_pos;
    if (!b->ran) return BIGSI_OK;
    TRY(need_run(b));          // waits for this batch's completion event
    TRY(host_counts(b));
    out->exact = b->exact ? 1 : 0;
    out->count_bytes = b->count_bytes;
    for (uint32_t v : b->h_num_unique) out->total_unique += v;
    uint64_t total = 0;
    if (b->fused_run) HIP_TRY(hipMemcpy(&total, b->hits.alloc.as<unsigned long long>() + (b->hits.gen & 1u), 8, hipMemcpyDeviceToHost));
    else if (b->compacted) HIP_TRY(hipMemcpy(&total, b->hits.hit_off.as<uint64_t>() + b->n_seqs, 8, hipMemcpyDeviceToHost));
    out->total_hits = total;
    out->bitmap_stride_bytes = b->wv_pad * 8;
    out->counts_stride = b->wv_pad * 64;
    out->d_bitmaps = b->bit_vectors();
    out->d_counts = b->counters();
    out->d_num_unique = b->num_unique.p;
    out->one_launch = b->fused_run ? 1 : 0;
    return BIGSI_OK;
}

extern "C" int bigsi_hip_batch_fetch_unique(bigsi_hip_batch *b, uint32_t *num_kmers, uint32_t *num_unique, uint32_t *min_kmers)
{
    BIGSI_ENTER(b ? b->ix : nullptr);
    TRY(need_run(b));
    TRY(host_counts(b));
    if (num_kmers) memcpy(num_kmers, b->h_num_kmers.data(), b->n_seqs * 4ull);
    if (num_unique) memcpy(num_unique, b->h_num_unique.data(), b->n_seqs * 4ull);
    if (min_kmers) memcpy(min_kmers, b->h_min_kmers.data(), b->n_seqs * 4ull);
    return BIGSI_OK;
}

extern "C" int bigsi_hip_batch_fetch_hits(bigsi_hip_batch *b, uint64_t *hit_offsets, uint32_t *colours, uint32_t *counts, uint64_t capacity)
{
    BIGSI_ENTER(b ? b->ix : nullptr);
    TRY(need_run(b));
    if (!b->compacted) {   // the run skipped K4: do it now
        TRY(compact_local(b, false));
        HIP_TRY(hipStreamSynchronize(b->ix->stream));
        b->compacted = true;
    }
    return fetch_hits_from(b, false, hit_offsets, colours, counts, capacity);
}

// Both gathered entries (`own_shard` null: bigsi_hip_batch_compact_gathered, which has no counters to fill in).  The compaction is
// queued behind the batch's run through its `done` event: no host-side wait, so the caller can go on to launch the next batch
// while this one's row-AND kernel is still running
static int queue_gathered(bigsi_hip_batch *b, const void *d_gathered, uint32_t n_shards, uint64_t shard_cols, const uint32_t *own_shard)
{
    if (!b) return fail(BIGSI_ERR_INVALID, "NULL batch");
    if (!b->ran) return fail(BIGSI_ERR_STATE, "bigsi_hip_batch_run has not completed for this batch");
    if (!b->exact && !own_shard)
        return fail(BIGSI_ERR_STATE, "the last run was thresholded: its shards exchange hit masks, which bigsi_hip_batch_compact_gathered_masks compacts");
    if (!d_gathered || n_shards == 0 || (own_shard && *own_shard >= n_shards)) return fail(BIGSI_ERR_INVALID, "bad gathered buffer / shard");
    if ((uint64_t)n_shards * shard_cols > 0xFFFFFFFFull) return fail(BIGSI_ERR_INVALID, "more than 2^32-1 colours in total");
    TRY(use_device(b->ix));
    hipStream_t st = b->gstream ? b->gstream : b->ix->stream;
    if (b->done) HIP_TRY(hipStreamWaitEvent(st, b->done, 0));
    b->g_src = d_gathered;
    b->g_shards = n_shards;
    b->g_shard_cols = shard_cols;
    b->g_own = b->exact ? kAllShards : *own_shard;
    EventPair ep{};
    TRY(ev_begin(b->ix, &ep, st));
    TRY(compact_gathered(b, false));
    TRY(ev_end(b->ix, &ep, b->ix->ev_cp, st));
    if (!b->g_done) HIP_TRY(hipEventCreateWithFlags(&b->g_done, hipEventDisableTiming));
    HIP_TRY(hipEventRecord(b->g_done, st));
    return BIGSI_OK;
}

extern "C" int bigsi_hip_batch_compact_gathered(bigsi_hip_batch *b, const void *d_gathered, uint32_t n_shards, uint64_t shard_cols)
{
    BIGSI_ENTER(b ? b->ix : nullptr);
    return queue_gathered(b, d_gathered, n_shards, shard_cols, nullptr);
}

extern "C" int bigsi_hip_batch_compact_gathered_masks(bigsi_hip_batch *b, const void *d_gathered_masks, uint32_t n_shards, uint64_t shard_cols,
                                                      uint32_t own_shard)
{
    BIGSI_ENTER(b ? b->ix : nullptr);
    return queue_gathered(b, d_gathered_masks, n_shards, shard_cols, &own_shard);
}

extern "C" int bigsi_hip_batch_set_gathered_hit_outputs(bigsi_hip_batch *b, void *d_colours, void *d_counts, uint64_t capacity)
{
    BIGSI_ENTER(b ? b->ix : nullptr);
    if (!b) return fail(BIGSI_ERR_INVALID, "NULL batch");
    if ((d_colours == nullptr) != (d_counts == nullptr)) return fail(BIGSI_ERR_INVALID, "give both buffers or neither");
    b->ghits.xcol = (uint32_t *)d_colours;
    b->ghits.xcnt = (uint32_t *)d_counts;
    b->ghits.xcap = d_colours ? capacity : 0;
    return BIGSI_OK;
}

extern "C" int bigsi_hip_batch_set_gather_stream(bigsi_hip_batch *b, void *hip_stream)
{
    BIGSI_ENTER(b ? b->ix : nullptr);
    if (!b) return fail(BIGSI_ERR_INVALID, "NULL batch");
    b->gstream = (hipStream_t)hip_stream;
    return BIGSI_OK;
}

extern "C" int bigsi_hip_batch_fetch_gathered_hits(bigsi_hip_batch *b, uint64_t *hit_offsets, uint32_t *colours, uint32_t *counts, uint64_t capacity)
{
    BIGSI_ENTER(b ? b->ix : nullptr);
    TRY(need_run(b));
    if (!b->g_src) return fail(BIGSI_ERR_STATE, "bigsi_hip_batch_compact_gathered has not been called");
    return fetch_hits_from(b, true, hit_offsets, colours, counts, capacity);
}

extern "C" int bigsi_hip_batch_fetch_counts(bigsi_hip_batch *b, uint32_t seq, uint32_t *out)
{
    BIGSI_ENTER(b ? b->ix : nullptr);
    TRY(need_run(b));
    if (!out) return fail(BIGSI_ERR_INVALID, "out is NULL");
    if (b->exact) return fail(BIGSI_ERR_STATE, "the last run took the exact path; re-run with BIGSI_RUN_FORCE_COUNTS or threshold < 1");
    if (b->sparse_counts) return fail(BIGSI_ERR_STATE, "the last run used BIGSI_RUN_SPARSE_COUNTS: only counters of hits were stored");
    if (seq >= b->n_seqs) return fail(BIGSI_ERR_RANGE, "sequence %u out of range", seq);
    const uint64_t n = b->ix->n_cols, cstride = b->wv_pad * 64;
    const uint8_t *src = (const uint8_t *)b->counters() + (uint64_t)seq * cstride * b->count_bytes;
    if (b->count_bytes == 4) {
        HIP_TRY(hipMemcpy(out, src, n * 4, hipMemcpyDeviceToHost));
    } else {
        std::vector<uint16_t> tmp(n);
        HIP_TRY(hipMemcpy(tmp.data(), src, n * 2, hipMemcpyDeviceToHost));
        for (uint64_t i = 0; i < n; i++) out[i] = tmp[i];
    }
    return BIGSI_OK;
}

extern "C" int bigsi_hip_batch_fetch_bitmap(bigsi_hip_batch *b, uint32_t seq, uint8_t *out)
{
    BIGSI_ENTER(b ? b->ix : nullptr);
    TRY(need_run(b));
    if (!out) return fail(BIGSI_ERR_INVALID, "out is NULL");
    if (!b->exact) return fail(BIGSI_ERR_STATE, "the last run took the counting path");
    if (seq >= b->n_seqs) return fail(BIGSI_ERR_RANGE, "sequence %u out of range", seq);
    const uint8_t *src = (const uint8_t *)b->bit_vectors() + (uint64_t)seq * b->wv_pad * 8;
    HIP_TRY(hipMemcpy(out, src, b->ix->rb(), hipMemcpyDeviceToHost));
    return BIGSI_OK;
}

extern "C" int bigsi_hip_batch_fetch_rows(bigsi_hip_batch *b, uint32_t seq, uint64_t *rows, uint64_t capacity)
{
    BIGSI_ENTER(b ? b->ix : nullptr);
    TRY(need_run(b));
    if (seq >= b->n_seqs) return fail(BIGSI_ERR_RANGE, "sequence %u out of range", seq);
    TRY(host_counts(b));
    const uint64_t n = (uint64_t)b->h_num_unique[seq] * b->ix->h;
    if (n > capacity) return fail(BIGSI_ERR_CAPACITY, "rows buffer holds %llu, %llu needed", (unsigned long long)capacity, (unsigned long long)n);
    if (n) HIP_TRY(hipMemcpy(rows, b->rows.as<uint64_t>() + b->pos_off[seq] * b->ix->h, n * 8, hipMemcpyDeviceToHost));
    return BIGSI_OK;
}

// include/bigsi_hip_testing.h: the list K2 streamed, as the last run's K1 or k_sort_rows left it (one copy, no kernel)
extern "C" int bigsi_hip_batch_fetch_rows_sorted(bigsi_hip_batch *b, uint32_t seq, uint64_t *rows, uint64_t capacity, uint32_t *shift)
{
    BIGSI_ENTER(b ? b->ix : nullptr);
    TRY(need_run(b));
    if (!shift) return fail(BIGSI_ERR_INVALID, "NULL argument");
    if (seq >= b->n_seqs) return fail(BIGSI_ERR_RANGE, "sequence %u out of range", seq);
    if (b->rpath.sorted_by == BIGSI_SORTED_BY_NONE) return fail(BIGSI_ERR_STATE, "the last run made no address-ordered row list");
    TRY(host_counts(b));
    const uint64_t n = (uint64_t)b->h_num_unique[seq] * b->ix->h;
    if (n > capacity) return fail(BIGSI_ERR_CAPACITY, "rows buffer holds %llu, %llu needed", (unsigned long long)capacity, (unsigned long long)n);
    if (b->rpath.sorted_by == BIGSI_SORTED_BY_K1) {       // (k_kmerize_lds: as many buckets as the query's dedupe table has slots)
        const uint64_t pos = b->pos_off[seq + 1] - b->pos_off[seq];
        uint64_t tsize = 2;
        while (tsize < (uint64_t)b->sorted_tab_mult * pos) tsize <<= 1;
        *shift = sort_shift(b->ix->m, tsize);
    } else *shift = sort_shift(b->ix->m, kSortBuckets);
    if (n) HIP_TRY(hipMemcpy(rows, b->rows_sorted.as<uint64_t>() + b->pos_off[seq] * b->ix->h, n * 8, hipMemcpyDeviceToHost));
    return BIGSI_OK;
}

// include/bigsi_hip_testing.h: K1's per-position maps of one sequence (two copies, no kernel)
extern "C" int bigsi_hip_batch_fetch_positions(bigsi_hip_batch *b, uint32_t seq, uint32_t *rep, uint32_t *pos_unique, uint64_t capacity)
{
    BIGSI_ENTER(b ? b->ix : nullptr);
    TRY(need_run(b));
    if (seq >= b->n_seqs) return fail(BIGSI_ERR_RANGE, "sequence %u out of range", seq);
    if (b->elements) return fail(BIGSI_ERR_STATE, "a batch of explicit k-mers has no representatives");
    TRY(host_counts(b));
    const uint64_t n = b->h_num_kmers[seq];
    if (n > capacity) return fail(BIGSI_ERR_CAPACITY, "position buffers hold %llu, %llu needed", (unsigned long long)capacity, (unsigned long long)n);
    if (n && rep) HIP_TRY(hipMemcpy(rep, b->rep.as<uint32_t>() + b->pos_off[seq], n * 4, hipMemcpyDeviceToHost));
    if (n && pos_unique) HIP_TRY(hipMemcpy(pos_unique, b->pos_unique.as<uint32_t>() + b->pos_off[seq], n * 4, hipMemcpyDeviceToHost));
    return BIGSI_OK;
}

extern "C" int bigsi_hip_batch_lookup(bigsi_hip_batch *b, uint32_t seq, uint32_t *first_pos, uint8_t *out_rows, uint64_t capacity_rows)
{
    BIGSI_ENTER(b ? b->ix : nullptr);
    TRY(need_run(b));
    if (seq >= b->n_seqs) return fail(BIGSI_ERR_RANGE, "sequence %u out of range", seq);
    TRY(host_counts(b));
    bigsi_hip_index *ix = b->ix;
    const uint32_t u = b->h_num_unique[seq];
    if (u > capacity_rows) return fail(BIGSI_ERR_CAPACITY, "lookup buffer holds %llu rows, %u needed", (unsigned long long)capacity_rows, u);
    if (u == 0) return BIGSI_OK;
    const uint64_t wv = ix->wv(), rb = ix->rb();
    if (first_pos) HIP_TRY(hipMemcpy(first_pos, b->first_pos.as<uint32_t>() + b->pos_off[seq], u * 4ull, hipMemcpyDeviceToHost));
    if (!out_rows) return BIGSI_OK;
    TRY(b->scratch.reserve((size_t)u * wv * 8));
    const uint64_t wblocks = ceil_div(wv, kBlock);
    if (wblocks * u > 0x7FFFFFFFull) return fail(BIGSI_ERR_INVALID, "lookup too large for one launch");
    hipLaunchKernelGGL(k_lookup, dim3((unsigned)(wblocks * u)), dim3(kBlock), 0, ix->stream, ix->d_index, ix->stride_words, (uint32_t)wv,
                       b->rows.as<uint64_t>() + b->pos_off[seq] * ix->h, ix->h, u, b->scratch.as<uint64_t>());
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpy2DAsync(out_rows, rb, b->scratch.p, wv * 8, rb, u, hipMemcpyDeviceToHost, ix->stream));
    HIP_TRY(hipStreamSynchronize(ix->stream));
    return BIGSI_OK;
}

extern "C" int bigsi_hip_batch_presence(bigsi_hip_batch *b, uint32_t seq, const uint32_t *colours, uint32_t n_colours, uint8_t *out)
{
    BIGSI_ENTER(b ? b->ix : nullptr);
    TRY(need_run(b));
    if (seq >= b->n_seqs) return fail(BIGSI_ERR_RANGE, "sequence %u out of range", seq);
    if (n_colours == 0) return BIGSI_OK;
    if (!colours || !out) return fail(BIGSI_ERR_INVALID, "NULL argument");
    bigsi_hip_index *ix = b->ix;
    for (uint32_t i = 0; i < n_colours; i++)
        if (colours[i] >= ix->n_cols) return fail(BIGSI_ERR_RANGE, "colour %u >= num_cols", colours[i]);
    TRY(host_counts(b));
    const uint32_t n = b->h_num_kmers[seq];
    if (n == 0) return BIGSI_OK;
    const size_t cbytes = round_up((size_t)n_colours * 4, 256);
    TRY(b->scratch.reserve(cbytes + (size_t)n_colours * n));
    uint8_t *d_out = b->scratch.as<uint8_t>() + cbytes;
    HIP_TRY(hipMemcpyAsync(b->scratch.p, colours, n_colours * 4ull, hipMemcpyHostToDevice, ix->stream));
    if (ceil_div(n, kBlock) * n_colours > 0x7FFFFFFFull) return fail(BIGSI_ERR_INVALID, "presence request too large for one launch");
    hipLaunchKernelGGL(k_presence, dim3((unsigned)(ceil_div(n, kBlock) * n_colours)), dim3(kBlock), 0, ix->stream, ix->d_index, ix->stride_words,
                       b->rows.as<uint64_t>() + b->pos_off[seq] * ix->h, b->pos_unique.as<uint32_t>() + b->pos_off[seq], ix->h, n,
                       b->scratch.as<uint32_t>(), n_colours, d_out);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(out, d_out, (size_t)n_colours * n, hipMemcpyDeviceToHost, ix->stream));
    HIP_TRY(hipStreamSynchronize(ix->stream));
    return BIGSI_OK;
}

// K-mer prevalence (k_kmer_prevalence + k_kmer_prevalence_sum; launch shape: plan_kmer_prevalence): per k-mer position of a batch that
// has run, the number of samples that hold the k-mer, under a universe mask and, with `subset`, a second count under a subset mask.
// The batch's scratch holds, for this call only: the two device masks (universe AND valid columns; subset AND that), zero-padded to
// whole 1 KiB segments, the slices' partial counts and the per-position results that are copied out.  Both kernels go to the index
// stream and are timed with the presence kernels (bigsi_hip_set_profiling / bigsi_hip_stats: presence_ms).
template <int H>
static void prevalence_launch_as(const PrevalencePlan &p, bigsi_hip_batch *b, bool with_subset, const uint64_t *umask, const uint64_t *smask, uint32_t *partial)
{
    bigsi_hip_index *ix = b->ix;
#define BIGSI_PREVALENCE(SUBSET)                                                                                                        \
    hipLaunchKernelGGL((k_kmer_prevalence<H, SUBSET>), dim3((unsigned)p.grid), dim3(p.block), 0, ix->stream, ix->d_index, ix->stride_words, ix->wv(), \
                       b->rows.as<uint64_t>(), b->d_pos_off.as<uint64_t>(), b->num_unique.as<uint32_t>(), b->n_seqs, b->total_pos, ix->h, umask, smask, \
                       p.slices, p.segs_per_slice, p.segs, p.waves_per_slice, partial, p.partial_stride)
    if (with_subset) BIGSI_PREVALENCE(true);
    else BIGSI_PREVALENCE(false);
#undef BIGSI_PREVALENCE
}

static int prevalence_launch(bigsi_hip_batch *b, const uint8_t *universe, const uint8_t *subset, uint32_t *total, uint32_t *in_subset)
{
    bigsi_hip_index *ix = b->ix;
    if (b->total_pos == 0) return BIGSI_OK;
    if (b->run_h != ix->h) return fail(BIGSI_ERR_STATE, "num_hashes changed since this batch ran (%u then, %u now): run it again", b->run_h, ix->h);
    if (ix->wv() > ix->stride_words || ix->stride_words % kVec)
        return fail(BIGSI_ERR_STATE, "internal: %llu column words do not fit the row stride %llu", (unsigned long long)ix->wv(), (unsigned long long)ix->stride_words);
    TRY(host_counts(b));
    uint64_t total_unique = 0;
    for (uint32_t v : b->h_num_unique) total_unique += v;
    const PrevalencePlan p = plan_kmer_prevalence(b->total_pos, total_unique, ix->wv(), ix->h);
    const uint64_t sum_grid = ceil_div(b->total_pos, kBlock);
    if (p.grid == 0 || p.grid > 0x7FFFFFFFull || sum_grid > 0x7FFFFFFFull)
        return fail(BIGSI_ERR_INVALID, "batch too large for one prevalence launch (%llu positions)", (unsigned long long)b->total_pos);
    // the masks in the row format: byte i < row_bytes = universe (all ones without one), the bits behind the last column cleared;
    // everything from there to the end of the last segment zero
    const uint64_t rb = ix->rb(), mask_bytes = (uint64_t)p.segs * 64 * kVec * 8, n_masks = subset ? 2 : 1;
    std::vector<uint8_t> masks(n_masks * mask_bytes, 0);
    for (uint64_t i = 0; i < rb; i++) masks[i] = universe ? universe[i] : 0xFF;
    if (ix->n_cols & 7) masks[rb - 1] &= (uint8_t)(0xFF00u >> (ix->n_cols & 7));
    if (subset)
        for (uint64_t i = 0; i < rb; i++) masks[mask_bytes + i] = subset[i] & masks[i];
    const uint64_t per = subset ? 2 : 1;
    const size_t o_partial = round_up(n_masks * mask_bytes, 256), o_total = round_up(o_partial + p.partial_entries * per * 4, 256);
    const size_t o_sub = round_up(o_total + b->total_pos * 4, 256), bytes = o_sub + (subset ? b->total_pos * 4 : 0);
    TRY(b->scratch.reserve(bytes));
    uint8_t *d = b->scratch.as<uint8_t>();
    const uint64_t *umask = reinterpret_cast<const uint64_t *>(d), *smask = subset ? reinterpret_cast<const uint64_t *>(d + mask_bytes) : nullptr;
    uint32_t *partial = reinterpret_cast<uint32_t *>(d + o_partial), *d_total = reinterpret_cast<uint32_t *>(d + o_total);
    uint32_t *d_sub = subset ? reinterpret_cast<uint32_t *>(d + o_sub) : nullptr;
    HIP_TRY(hipMemcpyAsync(d, masks.data(), masks.size(), hipMemcpyHostToDevice, ix->stream));
    EventPair ep{};
    TRY(bigsi_ev_begin(ix, &ep));
    switch (ix->h) {
    case 1: prevalence_launch_as<1>(p, b, subset != nullptr, umask, smask, partial); break;
    case 2: prevalence_launch_as<2>(p, b, subset != nullptr, umask, smask, partial); break;
    case 3: prevalence_launch_as<3>(p, b, subset != nullptr, umask, smask, partial); break;
    case 4: prevalence_launch_as<4>(p, b, subset != nullptr, umask, smask, partial); break;
    case 5: prevalence_launch_as<5>(p, b, subset != nullptr, umask, smask, partial); break;
    case 6: prevalence_launch_as<6>(p, b, subset != nullptr, umask, smask, partial); break;
    case 7: prevalence_launch_as<7>(p, b, subset != nullptr, umask, smask, partial); break;
    default: prevalence_launch_as<0>(p, b, subset != nullptr, umask, smask, partial); break;
    }
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(k_kmer_prevalence_sum, dim3((unsigned)sum_grid), dim3(kBlock), 0, ix->stream, partial, p.partial_stride, p.slices,
                       b->d_pos_off.as<uint64_t>(), b->n_seqs, b->pos_unique.as<uint32_t>(), b->total_pos, d_total, d_sub);
    HIP_TRY(hipGetLastError());
    TRY(bigsi_ev_end(ix, &ep, ix->ev_pr, nullptr, 2));
    HIP_TRY(hipMemcpyAsync(total, d_total, b->total_pos * 4, hipMemcpyDeviceToHost, ix->stream));
    if (subset) HIP_TRY(hipMemcpyAsync(in_subset, d_sub, b->total_pos * 4, hipMemcpyDeviceToHost, ix->stream));
    HIP_TRY(hipStreamSynchronize(ix->stream));          // (`masks` is read by its copy until here)
    return BIGSI_OK;
}

static int check_prevalence_args(const uint8_t *subset, const uint32_t *total, const uint32_t *in_subset)
{
    if (!total) return fail(BIGSI_ERR_INVALID, "total is NULL");
    if (in_subset && !subset) return fail(BIGSI_ERR_INVALID, "in_subset given without a subset mask");
    if (subset && !in_subset) return fail(BIGSI_ERR_INVALID, "a subset mask given without in_subset");
    return BIGSI_OK;
}

extern "C" int bigsi_hip_batch_kmer_prevalence(bigsi_hip_batch *b, const uint8_t *universe, const uint8_t *subset, uint32_t *total,
                                               uint32_t *in_subset, uint64_t capacity)
{
    BIGSI_ENTER(b ? b->ix : nullptr);
    TRY(need_run(b));
    TRY(check_prevalence_args(subset, total, in_subset));
    if (b->elements) return fail(BIGSI_ERR_STATE, "k-mer prevalence is not available for a batch of explicit k-mers");
    if (capacity < b->total_pos)
        return fail(BIGSI_ERR_CAPACITY, "prevalence buffers hold %llu entries, %llu needed", (unsigned long long)capacity, (unsigned long long)b->total_pos);
    return prevalence_launch(b, universe, subset, total, in_subset);
}

// The sequences are staged into a workspace of the index and run as an exact search: the exact row-AND is the cheapest run that leaves
// K1's arrays behind on every K1 route, and bigsi_batch_run stays as it is (a K1-only run is the follow-up: DESIGN.md).
extern "C" int bigsi_hip_kmer_prevalence(bigsi_hip_index *ix, const char *seqs, const uint64_t *offsets, uint32_t n_seqs, uint32_t k,
                                         const uint8_t *universe, const uint8_t *subset, uint64_t *pos_offsets, uint32_t *total,
                                         uint32_t *in_subset, uint64_t capacity)
{
    BIGSI_ENTER(ix);
    TRY(check_batch_args(ix, seqs, offsets, n_seqs, k));
    if (!pos_offsets) return fail(BIGSI_ERR_INVALID, "pos_offsets is NULL");
    TRY(check_prevalence_args(subset, total, in_subset));
    pos_offsets[0] = 0;
    for (uint32_t i = 0; i < n_seqs; i++) {
        const uint64_t len = offsets[i + 1] - offsets[i];
        pos_offsets[i + 1] = pos_offsets[i] + (len >= k ? len - k + 1 : 0);
    }
    if (capacity < pos_offsets[n_seqs])
        return fail(BIGSI_ERR_CAPACITY, "prevalence buffers hold %llu entries, %llu needed", (unsigned long long)capacity, (unsigned long long)pos_offsets[n_seqs]);
    // (the workspace is never a one-call batch: its run uploads the staging and records its event, so K1 leaves the device copy of pos_off)
    TRY(bigsi_batch_stage(ix, &ix->prevalence_ws, seqs, offsets, n_seqs, k));
    bigsi_hip_batch *b = ix->prevalence_ws;
    int rc = bigsi_batch_run(b, 1.0, 0, false);
    if (rc == BIGSI_OK) rc = need_run(b);
    if (rc == BIGSI_OK) rc = prevalence_launch(b, universe, subset, total, in_subset);
    if (rc != BIGSI_OK) drop_workspace(ix->prevalence_ws);
    return rc;
}

// Windowed search (include/bigsi_hip_window.h; k_window_max + k_window_combine, launch shape: plan_window_search; K4's k_hits_totals /
// k_hits_write on buffers of its own; k_window_bits + k_window_locate): per sample the best window of a batch that has run.  The
// batch's scratch holds, for this call only: segments | segment offsets | need | the segments' maxima | hit bitmap | uint16 counters |
// hit offsets | K4's group totals.  The hit lists go to win_col / win_cnt (the batch's own hit lists stay as its run left them), the
// locate pass's word offsets, presence words and records to win_loc.  Everything goes to the index stream and is timed with the
// presence kernels (bigsi_hip_set_profiling / bigsi_hip_stats: presence_ms).
template <int P, int H>
static void window_max_launch(const WindowPlan &p, bigsi_hip_batch *b, const WindowSeg *segs, uint64_t *partial)
{
    bigsi_hip_index *ix = b->ix;
    hipLaunchKernelGGL((k_window_max<P, H>), dim3((unsigned)p.grid), dim3(kBlock), 0, ix->stream, ix->d_index, ix->stride_words, (uint32_t)ix->wv(),
                       b->rows.as<uint64_t>(), b->d_pos_off.as<uint64_t>(), b->pos_unique.as<uint32_t>(), ix->h, segs, p.n_segs, p.tiles, partial, p.wvp);
}
template <int P>
static void window_max_launch_h(const WindowPlan &p, bigsi_hip_batch *b, const WindowSeg *segs, uint64_t *partial)
{
    switch (b->ix->h) {
    case 1: window_max_launch<P, 1>(p, b, segs, partial); break;
    case 2: window_max_launch<P, 2>(p, b, segs, partial); break;
    case 3: window_max_launch<P, 3>(p, b, segs, partial); break;
    case 4: window_max_launch<P, 4>(p, b, segs, partial); break;
    case 5: window_max_launch<P, 5>(p, b, segs, partial); break;
    case 6: window_max_launch<P, 6>(p, b, segs, partial); break;
    case 7: window_max_launch<P, 7>(p, b, segs, partial); break;
    default: window_max_launch<P, 0>(p, b, segs, partial); break;
    }
}

static int check_window_args(uint32_t window, double threshold, const uint32_t *window_used, const uint32_t *need, const uint64_t *hit_offsets,
                             const uint32_t *colours, const bigsi_hip_window_hit *records, uint64_t capacity)
{
    if (window == 0 || window > BIGSI_WINDOW_MAX) return fail(BIGSI_ERR_INVALID, "window must be 1 .. %u k-mer positions (got %u)", BIGSI_WINDOW_MAX, window);
    if (!(threshold > 0.0 && threshold <= 1.0)) return fail(BIGSI_ERR_INVALID, "threshold must be in (0, 1] (got %g)", threshold);
    if (!window_used || !need || !hit_offsets) return fail(BIGSI_ERR_INVALID, "window_used, need or hit_offsets is NULL");
    if (capacity && (!colours || !records)) return fail(BIGSI_ERR_INVALID, "colours or records is NULL");
    return BIGSI_OK;
}

// We and need of every sequence: ceil in IEEE double as min_kmers is derived (one multiply, as Python's math.ceil(We * t))
static void window_needs(const uint32_t *n, uint32_t n_seqs, uint32_t window, double threshold, uint32_t *window_used, uint32_t *need)
{
    for (uint32_t q = 0; q < n_seqs; q++) {
        const uint32_t we = std::min(n[q], window);
        window_used[q] = we;
        need[q] = (uint32_t)ceil((double)we * threshold);
    }
}

static int window_launch(bigsi_hip_batch *b, uint32_t window, double threshold, uint32_t *window_used, uint32_t *need, uint64_t *hit_offsets,
                         uint32_t *colours, bigsi_hip_window_hit *records, uint64_t capacity)
{
    static_assert(sizeof(bigsi_hip_window_hit) == sizeof(WindowRecord) && sizeof(WindowRecord) == 24, "the kernel's record is the header's");
    bigsi_hip_index *ix = b->ix;
    const uint32_t n_seqs = b->n_seqs;
    if (b->run_h != ix->h) return fail(BIGSI_ERR_STATE, "num_hashes changed since this batch ran (%u then, %u now): run it again", b->run_h, ix->h);
    if (ix->wv() > ix->stride_words || ix->stride_words % kVec)
        return fail(BIGSI_ERR_STATE, "internal: %llu column words do not fit the row stride %llu", (unsigned long long)ix->wv(), (unsigned long long)ix->stride_words);
    TRY(host_counts(b));
    window_needs(b->h_num_kmers.data(), n_seqs, window, threshold, window_used, need);
    memset(hit_offsets, 0, (n_seqs + 1) * 8ull);
    if (b->total_pos == 0 || ix->n_cols == 0) return BIGSI_OK;
    const uint64_t wv = ix->wv();
    const WindowPlan p = plan_window_search(b->h_num_kmers.data(), n_seqs, window, wv, ix->h, ix->window_starts, ix->window_cap);
    if (p.n_segs == 0) return BIGSI_OK;
    if (p.grid_too_large)
        return fail(BIGSI_ERR_INVALID, "window search too large for one launch: %llu segments x %u tiles = %llu workgroups (at most %llu)",
                    (unsigned long long)p.n_segs, p.tiles, (unsigned long long)p.grid, 0x7FFFFFFFull);
    if (p.partial_too_large)
        return fail(BIGSI_ERR_INVALID, "window search too large: %llu segments x %u planes x %llu words = %llu bytes of per-segment maxima (cap %llu)",
                    (unsigned long long)p.n_segs, p.planes, (unsigned long long)p.wvp, (unsigned long long)p.partial_bytes,
                    (unsigned long long)(ix->window_cap ? ix->window_cap : kWindowPartialBytes));
    const uint64_t bm_stride = p.wvp, out_stride = bm_stride * 64, counter_bytes = (uint64_t)n_seqs * out_stride * 2;
    if (counter_bytes > kWindowPartialBytes)
        return fail(BIGSI_ERR_INVALID, "window search too large: %u sequences x %llu columns = %llu bytes of counters (cap %llu): send fewer sequences per call",
                    n_seqs, (unsigned long long)out_stride, (unsigned long long)counter_bytes, (unsigned long long)kWindowPartialBytes);
    const uint32_t blocks_per_seq = (uint32_t)ceil_div(wv, kBlock);
    const uint64_t combine_grid = (uint64_t)blocks_per_seq * n_seqs;
    const uint32_t chunks = blocks_per_seq;
    const uint64_t nchunks = (uint64_t)chunks * n_seqs;
    if (combine_grid > 0x7FFFFFFFull) return fail(BIGSI_ERR_INVALID, "window search too large for one launch: %llu result words", (unsigned long long)combine_grid);

    // the call's tables, one upload: segments | segment offsets | need
    const size_t o_segoff = round_up(p.n_segs * sizeof(WindowSeg), 256), o_need = round_up(o_segoff + (n_seqs + 1) * 8ull, 256);
    const size_t o_partial = round_up(o_need + n_seqs * 4ull, 256), o_bm = round_up(o_partial + p.partial_bytes, 256);
    const size_t o_cnt = round_up(o_bm + (uint64_t)n_seqs * bm_stride * 8, 256), o_hoff = round_up(o_cnt + counter_bytes, 256);
    const size_t o_tot = round_up(o_hoff + (n_seqs + 1) * 8ull, 256), bytes = o_tot + kHitsMaxGroups * 4;
    std::vector<uint8_t> tables(o_partial, 0);
    memcpy(tables.data(), p.segs.data(), p.n_segs * sizeof(WindowSeg));
    memcpy(tables.data() + o_segoff, p.seg_off.data(), (n_seqs + 1) * 8ull);
    memcpy(tables.data() + o_need, need, n_seqs * 4ull);
    TRY(b->scratch.reserve(bytes));
    uint8_t *d = b->scratch.as<uint8_t>();
    HIP_TRY(hipMemcpy(d, tables.data(), tables.size(), hipMemcpyHostToDevice));
    const WindowSeg *d_segs = reinterpret_cast<const WindowSeg *>(d);
    const uint64_t *d_segoff = reinterpret_cast<const uint64_t *>(d + o_segoff);
    const uint32_t *d_need = reinterpret_cast<const uint32_t *>(d + o_need);
    uint64_t *d_partial = reinterpret_cast<uint64_t *>(d + o_partial), *d_bm = reinterpret_cast<uint64_t *>(d + o_bm);
    uint16_t *d_cnt = reinterpret_cast<uint16_t *>(d + o_cnt);
    uint64_t *d_hoff = reinterpret_cast<uint64_t *>(d + o_hoff);
    uint32_t *d_tot = reinterpret_cast<uint32_t *>(d + o_tot);
    if (b->win_cap == 0) {
        const uint64_t want = 1u << 16;
        TRY(b->win_col.reserve(want * 4));
        TRY(b->win_cnt.reserve(want * 4));
        b->win_cap = want;
    }

    EventPair ep{};
    TRY(bigsi_ev_begin(ix, &ep));
    switch (p.planes) {
    case 4: window_max_launch_h<4>(p, b, d_segs, d_partial); break;
    case 8: window_max_launch_h<8>(p, b, d_segs, d_partial); break;
    case 12: window_max_launch_h<12>(p, b, d_segs, d_partial); break;
    default: window_max_launch_h<16>(p, b, d_segs, d_partial); break;
    }
    HIP_TRY(hipGetLastError());
#define BIGSI_WINDOW_COMBINE(PL)                                                                                                       \
    hipLaunchKernelGGL((k_window_combine<PL>), dim3((unsigned)combine_grid), dim3(kBlock), 0, ix->stream, d_partial, p.wvp, d_segoff, n_seqs, \
                       (uint32_t)wv, blocks_per_seq, d_need, ix->n_cols, d_bm, bm_stride, d_cnt, out_stride)
    switch (p.planes) {
    case 4: BIGSI_WINDOW_COMBINE(4); break;
    case 8: BIGSI_WINDOW_COMBINE(8); break;
    case 12: BIGSI_WINDOW_COMBINE(12); break;
    default: BIGSI_WINDOW_COMBINE(16); break;
    }
#undef BIGSI_WINDOW_COMBINE
    HIP_TRY(hipGetLastError());
    // K4 as compact_bits launches it, on this call's bitmap and counters
    const HitsPlan hp = plan_hits(nchunks);
    const uint32_t ipb = hp.ipb;
    const uint64_t ngroups = hp.groups;
    auto hits_write = [&]() {
        hipLaunchKernelGGL(k_hits_write, dim3((unsigned)ngroups), dim3(kBlock), 0, ix->stream, (const uint64_t *)d_bm, bm_stride, (uint32_t)wv, n_seqs, 1u,
                           chunks, ix->n_cols, b->num_unique.as<uint32_t>(), ipb, d_tot, d_hoff, b->win_col.as<uint32_t>(), b->win_cnt.as<uint32_t>(),
                           b->win_cap, (const void *)d_cnt, 2u, out_stride, kAllShards, (uint64_t *)nullptr, 0u, (const uint32_t *)nullptr,
                           (volatile uint64_t *)nullptr, (uint64_t)0);
    };
    if (ngroups > 1)
        hipLaunchKernelGGL(k_hits_totals, dim3((unsigned)ngroups), dim3(kBlock), 0, ix->stream, (const uint64_t *)d_bm, bm_stride, (uint32_t)wv, n_seqs, 1u,
                           chunks, ipb, d_tot);
    hits_write();
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(hit_offsets, d_hoff, (n_seqs + 1) * 8ull, hipMemcpyDeviceToHost, ix->stream));
    HIP_TRY(hipStreamSynchronize(ix->stream));
    const uint64_t total = hit_offsets[n_seqs];
    if (total > capacity) {
        TRY(bigsi_ev_end(ix, &ep, ix->ev_pr, nullptr, 4));
        return fail(BIGSI_ERR_CAPACITY, "hit buffers hold %llu entries, %llu needed", (unsigned long long)capacity, (unsigned long long)total);
    }
    if (total == 0) return bigsi_ev_end(ix, &ep, ix->ev_pr, nullptr, 4);
    if (total > b->win_cap) {          // the write pass overflowed: grow the lists and run it again (the totals are still there)
        TRY(b->win_col.reserve(total * 4));
        TRY(b->win_cnt.reserve(total * 4));
        b->win_cap = total;
        hits_write();
        HIP_TRY(hipGetLastError());
    }
    // the locate pass: every hit's presence words, then its record
    std::vector<uint64_t> word_off(n_seqs + 1, 0);
    for (uint32_t q = 0; q < n_seqs; q++)
        word_off[q + 1] = word_off[q] + (hit_offsets[q + 1] - hit_offsets[q]) * ceil_div(b->h_num_kmers[q], 64);
    const uint64_t n_words = word_off[n_seqs], cap_bytes = ix->window_cap ? ix->window_cap : kWindowPartialBytes;
    if (n_words * 8 > cap_bytes || ceil_div(n_words, kBlock / 64) > 0x7FFFFFFFull) {
        TRY(bigsi_ev_end(ix, &ep, ix->ev_pr, nullptr, 4));
        return fail(BIGSI_ERR_INVALID, "window search too large: %llu hits need %llu bytes of presence bits (cap %llu): send fewer sequences per call or raise the threshold",
                    (unsigned long long)total, (unsigned long long)(n_words * 8), (unsigned long long)cap_bytes);
    }
    const size_t o_bits = round_up((n_seqs + 1) * 8ull, 256), o_rec = round_up(o_bits + n_words * 8, 256);
    TRY(b->win_loc.reserve(o_rec + total * sizeof(WindowRecord)));
    uint8_t *dl = b->win_loc.as<uint8_t>();
    HIP_TRY(hipMemcpy(dl, word_off.data(), (n_seqs + 1) * 8ull, hipMemcpyHostToDevice));
    const uint64_t *d_woff = reinterpret_cast<const uint64_t *>(dl);
    uint64_t *d_bits = reinterpret_cast<uint64_t *>(dl + o_bits);
    WindowRecord *d_rec = reinterpret_cast<WindowRecord *>(dl + o_rec);
    hipLaunchKernelGGL(k_window_bits, dim3((unsigned)ceil_div(n_words, kBlock / 64)), dim3(kBlock), 0, ix->stream, ix->d_index, ix->stride_words,
                       b->rows.as<uint64_t>(), b->d_pos_off.as<uint64_t>(), b->pos_unique.as<uint32_t>(), b->num_kmers.as<uint32_t>(), ix->h, n_seqs,
                       d_woff, (const uint64_t *)d_hoff, b->win_col.as<uint32_t>(), d_bits);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(k_window_locate, dim3((unsigned)ceil_div(total, kBlock / 64)), dim3(kBlock), 0, ix->stream, (const uint64_t *)d_bits, d_woff,
                       (const uint64_t *)d_hoff, n_seqs, b->num_kmers.as<uint32_t>(), d_need, window, d_rec);
    HIP_TRY(hipGetLastError());
    TRY(bigsi_ev_end(ix, &ep, ix->ev_pr, nullptr, 6));
    std::vector<uint32_t> h_col(total), h_cnt(total);
    std::vector<WindowRecord> h_rec(total);
    HIP_TRY(hipMemcpyAsync(h_col.data(), b->win_col.p, total * 4, hipMemcpyDeviceToHost, ix->stream));
    HIP_TRY(hipMemcpyAsync(h_cnt.data(), b->win_cnt.p, total * 4, hipMemcpyDeviceToHost, ix->stream));
    HIP_TRY(hipMemcpyAsync(h_rec.data(), d_rec, total * sizeof(WindowRecord), hipMemcpyDeviceToHost, ix->stream));
    HIP_TRY(hipStreamSynchronize(ix->stream));
    // the two device routes must agree before anything is handed out
    for (uint32_t q = 0; q < n_seqs; q++)
        for (uint64_t i = hit_offsets[q]; i < hit_offsets[q + 1]; i++)
            if (h_rec[i].best_found != h_cnt[i] || h_rec[i].best_found < need[q] || h_rec[i].windows_passing == 0)
                return fail(BIGSI_ERR_STATE, "internal: the two window kernels disagree on hit %llu (sequence %u, colour %u): sliding maximum %u, located %u in %u passing windows, need %u",
                            (unsigned long long)i, q, h_col[i], h_cnt[i], h_rec[i].best_found, h_rec[i].windows_passing, need[q]);
    memcpy(colours, h_col.data(), total * 4);
    memcpy(records, h_rec.data(), total * sizeof(WindowRecord));
    return BIGSI_OK;
}

extern "C" int bigsi_hip_batch_window_search(bigsi_hip_batch *b, uint32_t window, double threshold, uint32_t *window_used, uint32_t *need,
                                             uint64_t *hit_offsets, uint32_t *colours, bigsi_hip_window_hit *records, uint64_t capacity)
{
    BIGSI_ENTER(b ? b->ix : nullptr);
    TRY(need_run(b));
    TRY(check_window_args(window, threshold, window_used, need, hit_offsets, colours, records, capacity));
    if (b->elements) return fail(BIGSI_ERR_STATE, "a window search is not available for a batch of explicit k-mers");
    return window_launch(b, window, threshold, window_used, need, hit_offsets, colours, records, capacity);
}

// The sequences are staged into a workspace of the index and run as an exact search, as bigsi_hip_kmer_prevalence does: the exact
// row-AND is the cheapest run that leaves K1's arrays behind on every K1 route (a K1-only run is the follow-up: DESIGN.md).
extern "C" int bigsi_hip_window_search(bigsi_hip_index *ix, const char *seqs, const uint64_t *offsets, uint32_t n_seqs, uint32_t k, uint32_t window,
                                       double threshold, uint32_t *window_used, uint32_t *need, uint64_t *hit_offsets, uint32_t *colours,
                                       bigsi_hip_window_hit *records, uint64_t capacity)
{
    BIGSI_ENTER(ix);
    TRY(check_batch_args(ix, seqs, offsets, n_seqs, k));
    TRY(check_window_args(window, threshold, window_used, need, hit_offsets, colours, records, capacity));
    TRY(bigsi_batch_stage(ix, &ix->window_ws, seqs, offsets, n_seqs, k));
    bigsi_hip_batch *b = ix->window_ws;
    int rc = bigsi_batch_run(b, 1.0, 0, false);
    if (rc == BIGSI_OK) rc = need_run(b);
    if (rc == BIGSI_OK) rc = window_launch(b, window, threshold, window_used, need, hit_offsets, colours, records, capacity);
    if (rc != BIGSI_OK && rc != BIGSI_ERR_CAPACITY && rc != BIGSI_ERR_INVALID) drop_workspace(ix->window_ws);
    return rc;
}

extern "C" int bigsi_hip_window_set_limits(bigsi_hip_index *ix, uint64_t starts_per_segment, uint64_t partial_bytes_cap)
{
    BIGSI_ENTER(ix);
    if (!ix) return fail(BIGSI_ERR_INVALID, "NULL index");
    if (starts_per_segment >= (1ull << 31)) return fail(BIGSI_ERR_INVALID, "starts_per_segment must be below 2^31 (got %llu)", (unsigned long long)starts_per_segment);
    ix->window_starts = starts_per_segment;
    ix->window_cap = partial_bytes_cap;
    return BIGSI_OK;
}

extern "C" int bigsi_hip_band_set_limits(bigsi_hip_index *ix, uint32_t windows, uint32_t segments_per_launch)
{
    BIGSI_ENTER(ix);
    if (!ix) return fail(BIGSI_ERR_INVALID, "NULL index");
    if (windows > kBandMaxWindows || segments_per_launch > 2)
        return fail(BIGSI_ERR_INVALID, "at most %u windows and 2 segments per launch (got %u, %u)", kBandMaxWindows, windows, segments_per_launch);
    ix->band_windows = windows;
    ix->band_segs = segments_per_launch;
    return BIGSI_OK;
}

// Consumers of result vectors (the tally and the classification below): kernels that read what a run made with BIGSI_RUN_SKIP_COMPACT
// leaves behind -- the per-query result vectors and, below threshold 1, the counters -- for one batch, or for a stream cut into chunks.
struct VectorConsumer {
    const char *noun, *every_hit;      // for the refusals: "a tally" "counts" every hit
    bool host_chunks_take_a_slot;      // consume_stream: a chunk that never goes to the device still advances the workspace slot
};
constexpr VectorConsumer kTallyConsumer = {"a tally", "counts", true};
constexpr VectorConsumer kClassifyConsumer = {"a classification", "weighs", false};

// a batch a consumer may read: a finished SKIP_COMPACT run of one whole index, as the index is now
static int check_consumer_batch(const bigsi_hip_batch *b, const VectorConsumer &who)
{
    if (!b->ran) return fail(BIGSI_ERR_STATE, "bigsi_hip_batch_run has not completed for this batch");
    if (b->compacted || b->fused_run)
        return fail(BIGSI_ERR_STATE, "the batch's last run built hit lists: %s takes a run made with BIGSI_RUN_SKIP_COMPACT", who.noun);
    if (b->limit) return fail(BIGSI_ERR_STATE, "the batch has a result limit (bigsi_hip_batch_set_limit): %s %s every hit", who.noun, who.every_hit);
    if (b->ext_bitmaps || b->result_cols || b->comm)
        return fail(BIGSI_ERR_STATE, "the batch has caller-owned bit vectors, a result width or a communicator: %s takes a batch of one whole index", who.noun);
    if (b->run_h != b->ix->h) return fail(BIGSI_ERR_STATE, "num_hashes changed since this batch ran (%u then, %u now): run it again", b->run_h, b->ix->h);
    if (b->wv != b->ix->wv()) return fail(BIGSI_ERR_STATE, "num_cols changed since this batch ran: run it again");
    return BIGSI_OK;
}

// the stream a consumer's kernels go to: behind the batch's run, the last thing queued on its run stream
static hipStream_t consumer_stream(const bigsi_hip_batch *b) { return b->run_stream ? b->run_stream : b->ix->stream; }

// The run's counters -> the template instance <CountT, EXACT> a consumer kernel is compiled for: f(EXACT tag, typed counter pointer)
template <typename F>
static void with_counters(const bigsi_hip_batch *b, F &&f)
{
    if (b->exact) f(std::true_type{}, (const uint16_t *)nullptr);
    else if (b->count_bytes == 2) f(std::false_type{}, static_cast<const uint16_t *>(b->counters()));
    else f(std::false_type{}, static_cast<const uint32_t *>(b->counters()));
}

// The ordering rule, behind a consumer's last kernel on `st`: the batch's completion event is recorded again there, so whatever waits
// for the run -- reload, destroy, a fetch -- then waits for the consumer's reads of the batch's arrays too.  (finish_run's other
// fields hold their values already: a batch that passed check_consumer_batch has ran set and dirty clear.)
static int finish_consumer(bigsi_hip_batch *b, hipStream_t st)
{
    b->idle = false;
    return finish_run(b, st, false, st == b->ix->stream);
}

// the arguments of a stream call, all offsets included, before any device work
static int check_stream_args(const char *seqs, const uint64_t *offsets, uint64_t n_seqs, uint32_t k, double threshold)
{
    if (n_seqs == 0) return fail(BIGSI_ERR_INVALID, "a batch needs at least one sequence");
    if (k == 0) return fail(BIGSI_ERR_INVALID, "k must be > 0");
    if (!(threshold <= 1.0)) return fail(BIGSI_ERR_INVALID, "threshold must be <= 1, got %g", threshold);
    for (uint64_t i = 0; i < n_seqs; i++)
        if (offsets[i + 1] < offsets[i]) return fail(BIGSI_ERR_INVALID, "offsets must be non-decreasing");
    if (offsets[n_seqs] - offsets[0] && !seqs) return fail(BIGSI_ERR_INVALID, "seqs is NULL");
    return BIGSI_OK;
}

// A stream through two workspaces of the index (`ws`: the consumer's own, never the search stream's or another consumer's): chunk i is
// staged into workspace i & 1 -- host work, which first waits for that workspace's chunk i - 2 (its completion event, recorded behind
// its consumer kernels) -- while chunk i - 1 runs.  A chunk without any k-mer position never goes to the device: host_only(s0, s1).
// Every other chunk is run and handed over: launch(batch, slot, s0, s1).  A failed call gives both workspaces up.
template <typename HostOnly, typename Launch>
static int consume_stream(bigsi_hip_index *ix, bigsi_hip_batch *(&ws)[2], const VectorConsumer &who, const char *seqs, const uint64_t *offsets,
                          uint64_t n_seqs, uint32_t k, double threshold, HostOnly &&host_only, Launch &&launch)
{
    const bool exact = threshold == 1.0;
    const uint64_t wv_pad = round_up(ix->wv(), 2);
    int rc = BIGSI_OK;
    uint64_t chunk = 0;
    for (uint64_t s0 = 0; s0 < n_seqs && rc == BIGSI_OK;) {
        const uint64_t s1 = tally_chunk_end(offsets, n_seqs, s0, k, wv_pad, exact ? 0u : 4u);
        bool any_pos = false;
        for (uint64_t s = s0; s < s1 && !any_pos; s++) any_pos = offsets[s + 1] - offsets[s] >= k;
        if (!any_pos) host_only(s0, s1);
        else {
            const int slot = (int)(chunk & 1);
            rc = bigsi_batch_stage(ix, &ws[slot], seqs, offsets + s0, (uint32_t)(s1 - s0), k);
            // (hits-only counters below threshold 1: a consumer reads a counter only under a set bit, and a word that holds one keeps all 64)
            if (rc == BIGSI_OK) rc = bigsi_batch_run(ws[slot], threshold, BIGSI_RUN_SKIP_COMPACT | (exact ? 0u : (uint32_t)BIGSI_RUN_SPARSE_COUNTS), false);
            if (rc == BIGSI_OK) rc = check_consumer_batch(ws[slot], who);
            if (rc == BIGSI_OK) rc = launch(ws[slot], slot, s0, s1);
        }
        if (any_pos || who.host_chunks_take_a_slot) chunk++;
        s0 = s1;
    }
    if (rc != BIGSI_OK)
        for (bigsi_hip_batch *&w : ws) drop_workspace(w);
    return rc;
}

// Query-set tally (include/bigsi_hip_tally.h; k_tally_hits + k_tally_totals, launch shape: plan_tally): per-sample sums over the
// result vectors of runs made with BIGSI_RUN_SKIP_COMPACT.  One device allocation: queries_hit | kmers_found (wv * 64 entries each:
// a lane's column always has an entry, the ones behind num_cols stay zero) | totals[4].  `last` is recorded behind everything queued
// on behalf of the tally, on whichever stream it went to: reset and fetch wait for it, so a tally is in order with itself even when
// the index's stream is replaced between calls (bigsi_hip_set_stream).
struct bigsi_hip_tally {
    bigsi_hip_index *ix = nullptr;
    uint64_t n_cols = 0, m = 0, wv = 0;
    uint32_t h = 0;
    DevBuf acc;
    hipEvent_t last = nullptr;
    hipStream_t last_stream = nullptr;
    uint64_t host_skipped = 0;      // sequences of tally_add_stream chunks without any k-mer position: they never go to the device
    bool unusable = false;          // a tally_add_stream failed half way: until tally_reset
    uint64_t entries() const { return wv * 64; }
    unsigned long long *queries_hit() const { return acc.as<unsigned long long>(); }
    unsigned long long *kmers_found() const { return acc.as<unsigned long long>() + entries(); }
    unsigned long long *totals() const { return acc.as<unsigned long long>() + 2 * entries(); }
    size_t bytes() const { return (size_t)(2 * entries() + 4) * 8; }
};

static int tally_check(const bigsi_hip_tally *t, bool usable = true)
{
    const bigsi_hip_index *ix = t->ix;
    if (ix->n_cols != t->n_cols || ix->m != t->m || ix->h != t->h)
        return fail(BIGSI_ERR_STATE, "the index has changed since bigsi_hip_tally_create (%llu columns, %llu rows, %u hashes then; %llu, %llu, %u now)",
                    (unsigned long long)t->n_cols, (unsigned long long)t->m, t->h, (unsigned long long)ix->n_cols, (unsigned long long)ix->m, ix->h);
    if (usable && t->unusable) return fail(BIGSI_ERR_STATE, "a bigsi_hip_tally_add_stream on this tally failed half way: bigsi_hip_tally_reset starts over");
    return BIGSI_OK;
}

// what is queued on `st` next comes after everything queued on behalf of the tally so far
static int tally_order(bigsi_hip_tally *t, hipStream_t st)
{
    if (t->last && t->last_stream != st) HIP_TRY(hipStreamWaitEvent(st, t->last, 0));
    return BIGSI_OK;
}

static int tally_mark(bigsi_hip_tally *t, hipStream_t st)
{
    if (!t->last) HIP_TRY(hipEventCreateWithFlags(&t->last, hipEventDisableTiming));
    HIP_TRY(hipEventRecord(t->last, st));
    t->last_stream = st;
    return BIGSI_OK;
}

extern "C" int bigsi_hip_tally_create(bigsi_hip_index *ix, bigsi_hip_tally **out)
{
    BIGSI_ENTER(ix);
    if (!ix || !out) return fail(BIGSI_ERR_INVALID, "NULL argument");
    *out = nullptr;
    if (ix->n_cols == 0) return fail(BIGSI_ERR_STATE, "index has no columns");
    TRY(use_device(ix));
    bigsi_hip_tally *t = new (std::nothrow) bigsi_hip_tally();
    if (!t) return fail(BIGSI_ERR_NOMEM, "host allocation failed");
    t->ix = ix;
    t->n_cols = ix->n_cols; t->m = ix->m; t->h = ix->h; t->wv = ix->wv();
    int rc = t->acc.reserve(t->bytes());
    if (rc == BIGSI_OK) {
        hipError_t e = hipMemsetAsync(t->acc.p, 0, t->bytes(), ix->stream);
        if (e != hipSuccess) rc = fail(BIGSI_ERR_HIP, "hipMemsetAsync: %s", hipGetErrorString(e));
    }
    if (rc == BIGSI_OK) rc = tally_mark(t, ix->stream);
    if (rc != BIGSI_OK) { bigsi_hip_tally_destroy(t); return rc; }
    *out = t;
    return BIGSI_OK;
}

extern "C" int bigsi_hip_tally_destroy(bigsi_hip_tally *t)
{
    BusyGuard busy_guard_(t ? t->ix : nullptr, /*wait=*/true);
    if (!t) return BIGSI_OK;
    hipError_t e = hipSetDevice(t->ix->device);
    if (t->last) { e = hipEventSynchronize(t->last); e = hipEventDestroy(t->last); }
    (void)e;
    t->acc.release();
    delete t;
    return BIGSI_OK;
}

extern "C" int bigsi_hip_tally_reset(bigsi_hip_tally *t)
{
    BIGSI_ENTER(t ? t->ix : nullptr);
    if (!t) return fail(BIGSI_ERR_INVALID, "NULL tally");
    TRY(tally_check(t, false));
    TRY(use_device(t->ix));
    hipStream_t st = t->ix->stream;
    TRY(tally_order(t, st));
    HIP_TRY(hipMemsetAsync(t->acc.p, 0, t->bytes(), st));
    TRY(tally_mark(t, st));
    t->host_skipped = 0;
    t->unusable = false;
    return BIGSI_OK;
}

// the two kernels for a batch that passed check_consumer_batch (its result vectors are then as wide as the tally's), and finish_consumer
static int tally_launch(bigsi_hip_tally *t, bigsi_hip_batch *b)
{
    bigsi_hip_index *ix = b->ix;
    hipStream_t st = consumer_stream(b);
    const TallyPlan p = plan_tally(b->n_seqs, b->wv);
    if (p.too_large || p.totals_grid > 0x7FFFFFFFull)
        return fail(BIGSI_ERR_INVALID, "batch too large for one tally launch (%llu workgroups)", (unsigned long long)std::max(p.too_large, p.totals_grid));
    if (p.grid == 0) return BIGSI_OK;
    TRY(tally_order(t, st));
    const uint64_t *bm = static_cast<const uint64_t *>(b->bit_vectors());
    const uint64_t cstride = b->wv_pad * 64;
    EventPair ep{};
    TRY(bigsi_ev_begin(ix, &ep, st));
    with_counters(b, [&](auto exact, const auto *cnt) {
        using CountT = std::remove_const_t<std::remove_pointer_t<decltype(cnt)>>;
        hipLaunchKernelGGL((k_tally_hits<CountT, decltype(exact)::value>), dim3((unsigned)p.grid), dim3(p.block), 0, st, bm, b->wv_pad, (uint32_t)b->wv,
                           t->n_cols, b->n_seqs, b->num_unique.as<uint32_t>(), cnt, cstride, (uint32_t)p.word_groups, p.tile, t->queries_hit(),
                           t->kmers_found());
    });
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(k_tally_totals, dim3((unsigned)p.totals_grid), dim3(kBlock), 0, st, bm, b->wv_pad, (uint32_t)b->wv, t->n_cols, b->n_seqs,
                       b->num_unique.as<uint32_t>(), t->totals());
    HIP_TRY(hipGetLastError());
    TRY(bigsi_ev_end(ix, &ep, ix->ev_cp, st, 2));      // (timed with the compaction it stands in for: bigsi_hip_stats' compact_ms)
    TRY(tally_mark(t, st));
    return finish_consumer(b, st);
}

extern "C" int bigsi_hip_tally_add_batch(bigsi_hip_tally *t, bigsi_hip_batch *b)
{
    BIGSI_ENTER(t ? t->ix : nullptr);
    if (!t || !b) return fail(BIGSI_ERR_INVALID, "NULL argument");
    TRY(tally_check(t));
    if (b->ix != t->ix) return fail(BIGSI_ERR_STATE, "the batch belongs to another index than the tally");
    TRY(check_consumer_batch(b, kTallyConsumer));
    TRY(use_device(t->ix));
    return tally_launch(t, b);
}

// consume_stream over the index's tally_ws
extern "C" int bigsi_hip_tally_add_stream(bigsi_hip_tally *t, const char *seqs, const uint64_t *offsets, uint64_t n_seqs, uint32_t k, double threshold)
{
    BIGSI_ENTER(t ? t->ix : nullptr);
    if (!t || !offsets) return fail(BIGSI_ERR_INVALID, "NULL argument");
    TRY(tally_check(t));
    TRY(check_stream_args(seqs, offsets, n_seqs, k, threshold));
    const int rc = consume_stream(
        t->ix, t->ix->tally_ws, kTallyConsumer, seqs, offsets, n_seqs, k, threshold, [&](uint64_t s0, uint64_t s1) { t->host_skipped += s1 - s0; },
        [&](bigsi_hip_batch *b, int, uint64_t, uint64_t) { return tally_launch(t, b); });
    if (rc != BIGSI_OK) t->unusable = true;
    return rc;
}

extern "C" int bigsi_hip_tally_fetch(bigsi_hip_tally *t, uint64_t *queries_hit, uint64_t *kmers_found, uint64_t capacity, uint64_t totals[4])
{
    BIGSI_ENTER(t ? t->ix : nullptr);
    if (!t || !queries_hit || !kmers_found || !totals) return fail(BIGSI_ERR_INVALID, "NULL argument");
    TRY(tally_check(t));
    if (capacity < t->n_cols)
        return fail(BIGSI_ERR_CAPACITY, "tally buffers hold %llu entries, %llu needed", (unsigned long long)capacity, (unsigned long long)t->n_cols);
    TRY(use_device(t->ix));
    hipStream_t st = t->ix->stream;
    TRY(tally_order(t, st));
    uint64_t tot[4];
    HIP_TRY(hipMemcpyAsync(queries_hit, t->queries_hit(), t->n_cols * 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(kmers_found, t->kmers_found(), t->n_cols * 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(tot, t->totals(), sizeof tot, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    tot[2] += t->host_skipped;
    memcpy(totals, tot, sizeof tot);
    return BIGSI_OK;
}

// Read classification (include/bigsi_hip_classify.h; k_classify_groups, launch shape: plan_classify): per query the two best groups of
// samples over the result vectors of a run made with BIGSI_RUN_SKIP_COMPACT.  The index keeps the uploaded group_of, a device record
// buffer per stream slot and, for the stream call, a pinned twin and an event per slot.
static_assert(sizeof(bigsi_hip_classify_record) == 48, "record layout: three uint4 per query (k_classify_groups)");
constexpr bigsi_hip_classify_record kClassifyEmpty = {0, 0, 0, 0, BIGSI_CLASSIFY_NONE, 0, BIGSI_CLASSIFY_NONE, 0, BIGSI_CLASSIFY_NONE, 0, BIGSI_CLASSIFY_NONE, 0};

static int classify_check_groups(const bigsi_hip_index *ix, const uint32_t *group_of, uint64_t n_entries, uint32_t n_groups)
{
    if (ix->n_cols == 0) return fail(BIGSI_ERR_STATE, "index has no columns");
    if (n_entries != ix->n_cols)
        return fail(BIGSI_ERR_INVALID, "group_of has %llu entries, the index has %llu columns", (unsigned long long)n_entries, (unsigned long long)ix->n_cols);
    if (plan_classify(1, ix->wv(), n_groups).bad_groups) return fail(BIGSI_ERR_INVALID, "n_groups must be 1 .. %u (got %u)", kClassifyMaxGroups, n_groups);
    const uint64_t bad = classify_bad_column(group_of, n_entries, n_groups);
    if (bad != n_entries)
        return fail(BIGSI_ERR_INVALID, "group_of[%llu] = %u is neither below n_groups (%u) nor BIGSI_CLASSIFY_NONE", (unsigned long long)bad, group_of[bad], n_groups);
    return BIGSI_OK;
}

// the kernel for a batch that passed check_consumer_batch, on its consumer_stream `st`, its records into `slot`'s device buffer, and
// finish_consumer.  group_of is on the device already, ordered before the kernel.
static int classify_launch(bigsi_hip_batch *b, uint32_t n_groups, int slot, hipStream_t st)
{
    bigsi_hip_index *ix = b->ix;
    const ClassifyPlan p = plan_classify(b->n_seqs, b->wv, n_groups);
    if (p.too_large || p.bad_groups) return fail(BIGSI_ERR_INVALID, "batch too large for one classification launch (%llu workgroups)", (unsigned long long)p.too_large);
    TRY(ix->classify_rec[slot].reserve((size_t)b->n_seqs * sizeof(bigsi_hip_classify_record)));
    const uint64_t *bm = static_cast<const uint64_t *>(b->bit_vectors());
    const uint64_t cstride = b->wv_pad * 64;
    EventPair ep{};
    TRY(bigsi_ev_begin(ix, &ep, st));
    with_counters(b, [&](auto exact, const auto *cnt) {
        using CountT = std::remove_const_t<std::remove_pointer_t<decltype(cnt)>>;
        hipLaunchKernelGGL((k_classify_groups<CountT, decltype(exact)::value>), dim3((unsigned)p.grid), dim3(p.block), p.lds_bytes, st, bm, b->wv_pad,
                           (uint32_t)b->wv, ix->n_cols, b->num_unique.as<uint32_t>(), b->threshold, cnt, cstride, ix->classify_groups.as<uint32_t>(),
                           n_groups, p.table_bytes, ix->classify_rec[slot].as<uint4>());
    });
    HIP_TRY(hipGetLastError());
    TRY(bigsi_ev_end(ix, &ep, ix->ev_cp, st, 1));      // (timed with the compaction it stands in for: bigsi_hip_stats' compact_ms)
    return finish_consumer(b, st);
}

extern "C" int bigsi_hip_classify_batch(bigsi_hip_batch *b, const uint32_t *group_of, uint64_t n_entries, uint32_t n_groups,
                                        bigsi_hip_classify_record *records, uint64_t capacity)
{
    BIGSI_ENTER(b ? b->ix : nullptr);
    if (!b || !group_of || !records) return fail(BIGSI_ERR_INVALID, "NULL argument");
    bigsi_hip_index *ix = b->ix;
    TRY(classify_check_groups(ix, group_of, n_entries, n_groups));
    TRY(check_consumer_batch(b, kClassifyConsumer));
    if (capacity < b->n_seqs)
        return fail(BIGSI_ERR_CAPACITY, "the record buffer holds %llu entries, %u needed", (unsigned long long)capacity, b->n_seqs);
    TRY(use_device(ix));
    hipStream_t st = consumer_stream(b);
    TRY(ix->classify_groups.reserve((size_t)n_entries * 4));
    HIP_TRY(hipMemcpyAsync(ix->classify_groups.p, group_of, (size_t)n_entries * 4, hipMemcpyHostToDevice, st));
    TRY(classify_launch(b, n_groups, 0, st));
    HIP_TRY(hipMemcpyAsync(records, ix->classify_rec[0].p, (size_t)b->n_seqs * sizeof(bigsi_hip_classify_record), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    return BIGSI_OK;
}

// consume_stream over the index's classify_ws: the records of chunk i - 1 are collected (its slot's event, then a host copy out of the
// pinned twin) once chunk i is queued.
static int classify_collect(bigsi_hip_index *ix, int slot, bigsi_hip_classify_record *dst, uint64_t n)
{
    HIP_TRY(hipEventSynchronize(ix->classify_ev[slot]));
    memcpy(dst, ix->classify_pin[slot], (size_t)n * sizeof(bigsi_hip_classify_record));
    return BIGSI_OK;
}

extern "C" int bigsi_hip_classify_stream(bigsi_hip_index *ix, const char *seqs, const uint64_t *offsets, uint64_t n_seqs, uint32_t k, double threshold,
                                         const uint32_t *group_of, uint64_t n_entries, uint32_t n_groups, bigsi_hip_classify_record *records)
{
    BIGSI_ENTER(ix);
    if (!ix || !offsets || !group_of || !records) return fail(BIGSI_ERR_INVALID, "NULL argument");
    TRY(check_stream_args(seqs, offsets, n_seqs, k, threshold));
    TRY(classify_check_groups(ix, group_of, n_entries, n_groups));
    TRY(use_device(ix));
    const size_t slot_bytes = (size_t)kTallyChunkSeqs * sizeof(bigsi_hip_classify_record);
    for (int s = 0; s < 2; s++) {
        if (!ix->classify_pin[s]) HIP_TRY(hipHostMalloc(&ix->classify_pin[s], slot_bytes, hipHostMallocDefault));
        if (!ix->classify_ev[s]) HIP_TRY(hipEventCreateWithFlags(&ix->classify_ev[s], hipEventDisableTiming));
    }
    TRY(ix->classify_groups.reserve((size_t)n_entries * 4));
    HIP_TRY(hipMemcpyAsync(ix->classify_groups.p, group_of, (size_t)n_entries * 4, hipMemcpyHostToDevice, ix->stream));
    HIP_TRY(hipStreamSynchronize(ix->stream));      // (a pageable source: the upload is over before the caller's array can change, whichever stream a chunk runs on)
    uint64_t pend_s0 = 0, pend_n = 0;      // the chunk whose records are still on their way: slot pend_slot
    int pend_slot = -1;
    int rc = consume_stream(
        ix, ix->classify_ws, kClassifyConsumer, seqs, offsets, n_seqs, k, threshold,
        [&](uint64_t s0, uint64_t s1) { std::fill(records + s0, records + s1, kClassifyEmpty); },
        [&](bigsi_hip_batch *b, int slot, uint64_t s0, uint64_t s1) -> int {
            hipStream_t st = consumer_stream(b);
            TRY(classify_launch(b, n_groups, slot, st));
            hipError_t e = hipMemcpyAsync(ix->classify_pin[slot], ix->classify_rec[slot].p, (size_t)(s1 - s0) * sizeof(bigsi_hip_classify_record), hipMemcpyDeviceToHost, st);
            if (e == hipSuccess) e = hipEventRecord(ix->classify_ev[slot], st);
            if (e != hipSuccess) return fail(BIGSI_ERR_HIP, "queueing the record download: %s", hipGetErrorString(e));
            if (pend_slot >= 0) TRY(classify_collect(ix, pend_slot, records + pend_s0, pend_n));
            pend_slot = slot; pend_s0 = s0; pend_n = s1 - s0;
            return BIGSI_OK;
        });
    if (rc == BIGSI_OK && pend_slot >= 0) {
        rc = classify_collect(ix, pend_slot, records + pend_s0, pend_n);
        if (rc != BIGSI_OK)
            for (bigsi_hip_batch *&w : ix->classify_ws) drop_workspace(w);
    }
    return rc;
}

// Group association (include/bigsi_hip_associate.h; k_group_masks + k_group_counts, launch shape: plan_associate): per query every
// group's number of hit columns over the result vectors of a run made with BIGSI_RUN_SKIP_COMPACT.  The third consumer: no counter is
// read, so there is no with_counters here.  The index keeps the uploaded group_of, the masks built from it, a device output buffer
// per stream slot (a chunk's infos, its counts behind them) and, for the stream call, a pinned twin and an event per slot.
static_assert(sizeof(bigsi_hip_associate_info) == 16, "info layout: one uint4 per query (k_group_counts)");
static_assert(BIGSI_ASSOCIATE_NONE == kAssociateNoGroup && BIGSI_ASSOCIATE_MAX_GROUPS == kAssociateMaxGroups, "header and planner");
constexpr VectorConsumer kAssociateConsumer = {"an association", "counts", false};

// classify_check_groups' rules and message shapes under this header's names; then group_of goes up and the masks are built, both on `st`
static int associate_groups(bigsi_hip_index *ix, const uint32_t *group_of, uint64_t n_entries, uint32_t n_groups)
{
    if (ix->n_cols == 0) return fail(BIGSI_ERR_STATE, "index has no columns");
    if (n_entries != ix->n_cols)
        return fail(BIGSI_ERR_INVALID, "group_of has %llu entries, the index has %llu columns", (unsigned long long)n_entries, (unsigned long long)ix->n_cols);
    if (plan_associate(1, ix->wv(), n_groups).bad_groups)
        return fail(BIGSI_ERR_INVALID, "n_groups must be 1 .. BIGSI_ASSOCIATE_MAX_GROUPS = %u (got %u)", kAssociateMaxGroups, n_groups);
    const uint64_t bad = classify_bad_column(group_of, n_entries, n_groups);
    if (bad != n_entries)
        return fail(BIGSI_ERR_INVALID, "group_of[%llu] = %u is neither below n_groups (%u) nor BIGSI_ASSOCIATE_NONE", (unsigned long long)bad, group_of[bad], n_groups);
    return BIGSI_OK;
}

static int associate_masks(bigsi_hip_index *ix, const uint32_t *group_of, uint32_t n_groups, hipStream_t st)
{
    const AssociatePlan p = plan_associate(1, ix->wv(), n_groups);
    if (p.too_large) return fail(BIGSI_ERR_INVALID, "index too wide for one mask launch (%llu workgroups)", (unsigned long long)p.too_large);
    TRY(ix->associate_groups.reserve((size_t)ix->n_cols * 4));
    TRY(ix->associate_masks.reserve((size_t)p.mask_bytes));
    HIP_TRY(hipMemcpyAsync(ix->associate_groups.p, group_of, (size_t)ix->n_cols * 4, hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(k_group_masks, dim3((unsigned)p.mask_grid), dim3(p.block), 0, st, ix->associate_groups.as<uint32_t>(), ix->n_cols, (uint32_t)ix->wv(),
                       n_groups, ix->associate_masks.as<uint64_t>());
    HIP_TRY(hipGetLastError());
    return BIGSI_OK;
}

// the count kernel for a batch that passed check_consumer_batch, on its consumer_stream `st`, its outputs into `slot`'s device buffer
// (info[n_seqs] | counts[n_seqs][n_groups]: the uint4 stores stay aligned), and finish_consumer.  The masks are on the device already, ordered before the kernel.
static int associate_launch(bigsi_hip_batch *b, uint32_t n_groups, int slot, hipStream_t st)
{
    bigsi_hip_index *ix = b->ix;
    const AssociatePlan p = plan_associate(b->n_seqs, b->wv, n_groups);
    if (p.too_large || p.bad_groups) return fail(BIGSI_ERR_INVALID, "batch too large for one association launch (%llu workgroups)", (unsigned long long)p.too_large);
    const size_t info_bytes = (size_t)b->n_seqs * sizeof(bigsi_hip_associate_info);
    TRY(ix->associate_out[slot].reserve(info_bytes + (size_t)b->n_seqs * n_groups * 4));
    uint8_t *out = static_cast<uint8_t *>(ix->associate_out[slot].p);
    EventPair ep{};
    TRY(bigsi_ev_begin(ix, &ep, st));
    hipLaunchKernelGGL(k_group_counts, dim3((unsigned)p.grid), dim3(p.block), 0, st, static_cast<const uint64_t *>(b->bit_vectors()), b->wv_pad, (uint32_t)b->wv,
                       ix->n_cols, b->num_unique.as<uint32_t>(), b->threshold, (uint32_t)b->n_seqs, ix->associate_masks.as<uint64_t>(), n_groups,
                       reinterpret_cast<uint32_t *>(out + info_bytes), reinterpret_cast<uint4 *>(out));
    HIP_TRY(hipGetLastError());
    TRY(bigsi_ev_end(ix, &ep, ix->ev_cp, st, 1));      // (timed with the compaction it stands in for: bigsi_hip_stats' compact_ms)
    return finish_consumer(b, st);
}

extern "C" int bigsi_hip_associate_batch(bigsi_hip_batch *b, const uint32_t *group_of, uint64_t n_entries, uint32_t n_groups, uint32_t *counts,
                                         bigsi_hip_associate_info *info, uint64_t capacity)
{
    BIGSI_ENTER(b ? b->ix : nullptr);
    if (!b || !group_of || !counts || !info) return fail(BIGSI_ERR_INVALID, "NULL argument");
    bigsi_hip_index *ix = b->ix;
    TRY(associate_groups(ix, group_of, n_entries, n_groups));
    TRY(check_consumer_batch(b, kAssociateConsumer));
    if (capacity < b->n_seqs)
        return fail(BIGSI_ERR_CAPACITY, "the output buffers hold %llu sequences, %u needed", (unsigned long long)capacity, b->n_seqs);
    TRY(use_device(ix));
    hipStream_t st = consumer_stream(b);
    TRY(associate_masks(ix, group_of, n_groups, st));
    TRY(associate_launch(b, n_groups, 0, st));
    const size_t info_bytes = (size_t)b->n_seqs * sizeof(bigsi_hip_associate_info);
    const uint8_t *out = static_cast<const uint8_t *>(ix->associate_out[0].p);
    HIP_TRY(hipMemcpyAsync(info, out, info_bytes, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(counts, out + info_bytes, (size_t)b->n_seqs * n_groups * 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    return BIGSI_OK;
}

// consume_stream over the index's associate_ws: the outputs of chunk i - 1 are collected (its slot's event, then two host copies out of
// the pinned twin, which is laid out as the device buffer is) once chunk i is queued.
static int associate_collect(bigsi_hip_index *ix, int slot, uint32_t n_groups, uint32_t *counts, bigsi_hip_associate_info *info, uint64_t n)
{
    HIP_TRY(hipEventSynchronize(ix->associate_ev[slot]));
    const uint8_t *pin = static_cast<const uint8_t *>(ix->associate_pin[slot]);
    memcpy(info, pin, (size_t)n * sizeof(bigsi_hip_associate_info));
    memcpy(counts, pin + (size_t)n * sizeof(bigsi_hip_associate_info), (size_t)n * n_groups * 4);
    return BIGSI_OK;
}

extern "C" int bigsi_hip_associate_stream(bigsi_hip_index *ix, const char *seqs, const uint64_t *offsets, uint64_t n_seqs, uint32_t k, double threshold,
                                          const uint32_t *group_of, uint64_t n_entries, uint32_t n_groups, uint32_t *counts,
                                          bigsi_hip_associate_info *info)
{
    BIGSI_ENTER(ix);
    if (!ix || !offsets || !group_of || !counts || !info) return fail(BIGSI_ERR_INVALID, "NULL argument");
    TRY(check_stream_args(seqs, offsets, n_seqs, k, threshold));
    TRY(associate_groups(ix, group_of, n_entries, n_groups));
    TRY(use_device(ix));
    // (a slot for the largest chunk of the widest partition: kTallyChunkSeqs x (n_groups + 4) x 4 bytes at n_groups = 64, 1.1 MB)
    const size_t slot_bytes = (size_t)kTallyChunkSeqs * (kAssociateMaxGroups + 4) * 4;
    for (int s = 0; s < 2; s++) {
        if (!ix->associate_pin[s]) HIP_TRY(hipHostMalloc(&ix->associate_pin[s], slot_bytes, hipHostMallocDefault));
        if (!ix->associate_ev[s]) HIP_TRY(hipEventCreateWithFlags(&ix->associate_ev[s], hipEventDisableTiming));
    }
    TRY(associate_masks(ix, group_of, n_groups, ix->stream));
    HIP_TRY(hipStreamSynchronize(ix->stream));      // (a pageable source, and the masks are there whichever stream a chunk runs on)
    const size_t per_seq = ((size_t)n_groups + 4) * 4;
    uint64_t pend_s0 = 0, pend_n = 0;      // the chunk whose outputs are still on their way: slot pend_slot
    int pend_slot = -1;
    int rc = consume_stream(
        ix, ix->associate_ws, kAssociateConsumer, seqs, offsets, n_seqs, k, threshold,
        [&](uint64_t s0, uint64_t s1) {
            memset(counts + s0 * n_groups, 0, (size_t)(s1 - s0) * n_groups * 4);
            memset(info + s0, 0, (size_t)(s1 - s0) * sizeof(bigsi_hip_associate_info));
        },
        [&](bigsi_hip_batch *b, int slot, uint64_t s0, uint64_t s1) -> int {
            hipStream_t st = consumer_stream(b);
            TRY(associate_launch(b, n_groups, slot, st));
            hipError_t e = hipMemcpyAsync(ix->associate_pin[slot], ix->associate_out[slot].p, (size_t)(s1 - s0) * per_seq, hipMemcpyDeviceToHost, st);
            if (e == hipSuccess) e = hipEventRecord(ix->associate_ev[slot], st);
            if (e != hipSuccess) return fail(BIGSI_ERR_HIP, "queueing the count download: %s", hipGetErrorString(e));
            if (pend_slot >= 0) TRY(associate_collect(ix, pend_slot, n_groups, counts + pend_s0 * n_groups, info + pend_s0, pend_n));
            pend_slot = slot; pend_s0 = s0; pend_n = s1 - s0;
            return BIGSI_OK;
        });
    if (rc == BIGSI_OK && pend_slot >= 0) {
        rc = associate_collect(ix, pend_slot, n_groups, counts + pend_s0 * n_groups, info + pend_s0, pend_n);
        if (rc != BIGSI_OK)
            for (bigsi_hip_batch *&w : ix->associate_ws) drop_workspace(w);
    }
    return rc;
}

// Panel genotyping (include/bigsi_hip_genotype.h; k_allele_or + k_genotype_variants + k_genotype_samples, launch shapes:
// plan_genotype): the fourth consumer, a segmented OR of the result vectors into one plane per allele.  No counter is read.  The
// accumulator owns planes[2 n_variants][wv], used[2 n_variants], the selection vector sel[wv] (columns & valid_mask, built at create),
// the two count outputs of a fetch, and two staging slots for allele_of (pinned host + device): an add copies its entries into the
// slot of its turn and uploads from there, so the caller's array is not read after the call returns and no add waits for its own
// kernel.  `last` orders the accumulator with itself, as the tally's does.
static_assert(BIGSI_GENOTYPE_NONE == kGenotypeNone && BIGSI_GENOTYPE_MAX_VARIANTS == kGenotypeMaxVariants && BIGSI_GENOTYPE_PLANE_BYTES == kGenotypePlaneBytes,
              "header and planner");
constexpr VectorConsumer kGenotypeConsumer = {"a genotyping", "folds", false};

struct bigsi_hip_genotype {
    bigsi_hip_index *ix = nullptr;
    uint64_t n_cols = 0, m = 0, wv = 0;
    uint32_t h = 0, n_variants = 0, n_selected = 0;
    DevBuf planes, used, sel, variant_counts, sample_counts;
    DevBuf d_allele[2];
    void *pin[2] = {nullptr, nullptr};
    size_t pin_cap[2] = {0, 0};
    hipEvent_t pin_ev[2] = {nullptr, nullptr};      // behind the upload out of pin[slot]
    unsigned turn = 0;
    hipEvent_t last = nullptr;
    hipStream_t last_stream = nullptr;
    bool unusable = false;                          // a genotype_add_stream failed half way: until genotype_reset
    size_t plane_bytes() const { return (size_t)2 * n_variants * wv * 8; }
    uint64_t row_bytes() const { return (n_cols + 7) / 8; }
};

static int genotype_check(const bigsi_hip_genotype *g, bool usable = true)
{
    const bigsi_hip_index *ix = g->ix;
    if (ix->n_cols != g->n_cols || ix->m != g->m || ix->h != g->h)
        return fail(BIGSI_ERR_STATE, "the index has changed since bigsi_hip_genotype_create (%llu columns, %llu rows, %u hashes then; %llu, %llu, %u now)",
                    (unsigned long long)g->n_cols, (unsigned long long)g->m, g->h, (unsigned long long)ix->n_cols, (unsigned long long)ix->m, ix->h);
    if (usable && g->unusable)
        return fail(BIGSI_ERR_STATE, "a bigsi_hip_genotype_add_stream on this accumulator failed half way: bigsi_hip_genotype_reset starts over");
    return BIGSI_OK;
}

// what is queued on `st` next comes after everything queued on behalf of the accumulator so far
static int genotype_order(bigsi_hip_genotype *g, hipStream_t st)
{
    if (g->last && g->last_stream != st) HIP_TRY(hipStreamWaitEvent(st, g->last, 0));
    return BIGSI_OK;
}

static int genotype_mark(bigsi_hip_genotype *g, hipStream_t st)
{
    if (!g->last) HIP_TRY(hipEventCreateWithFlags(&g->last, hipEventDisableTiming));
    HIP_TRY(hipEventRecord(g->last, st));
    g->last_stream = st;
    return BIGSI_OK;
}

static int genotype_zero(bigsi_hip_genotype *g, hipStream_t st)
{
    HIP_TRY(hipMemsetAsync(g->planes.p, 0, g->plane_bytes(), st));
    HIP_TRY(hipMemsetAsync(g->used.p, 0, (size_t)2 * g->n_variants * 4, st));
    return genotype_mark(g, st);
}

extern "C" int bigsi_hip_genotype_create(bigsi_hip_index *ix, uint32_t n_variants, const uint8_t *columns, bigsi_hip_genotype **out)
{
    BIGSI_ENTER(ix);
    if (!ix || !out) return fail(BIGSI_ERR_INVALID, "NULL argument");
    *out = nullptr;
    if (ix->n_cols == 0) return fail(BIGSI_ERR_STATE, "index has no columns");
    const uint64_t wv = ix->wv();
    const GenotypePlan p = plan_genotype(1, wv, n_variants);
    if (p.bad_variants)
        return fail(BIGSI_ERR_INVALID, "n_variants must be 1 .. BIGSI_GENOTYPE_MAX_VARIANTS = %u (got %u)", kGenotypeMaxVariants, n_variants);
    if (p.too_many_bytes)
        return fail(BIGSI_ERR_NOMEM, "the planes of %u variants over %llu columns take 2 x %u x %llu x 8 bytes, above BIGSI_GENOTYPE_PLANE_BYTES = %llu: slice the panel by variant",
                    n_variants, (unsigned long long)ix->n_cols, n_variants, (unsigned long long)wv, (unsigned long long)kGenotypePlaneBytes);
    if (p.too_large || p.variants_grid > 0x7FFFFFFFull) return fail(BIGSI_ERR_INVALID, "index too wide for one genotype launch (%llu workgroups)", (unsigned long long)p.too_large);
    TRY(use_device(ix));
    bigsi_hip_genotype *g = new (std::nothrow) bigsi_hip_genotype();
    if (!g) return fail(BIGSI_ERR_NOMEM, "host allocation failed");
    g->ix = ix;
    g->n_cols = ix->n_cols; g->m = ix->m; g->h = ix->h; g->wv = wv;
    g->n_variants = n_variants;
    std::vector<uint64_t> sel(wv, columns ? 0ull : ~0ull);
    if (columns) memcpy(sel.data(), columns, g->row_bytes());      // (row format = the little-endian words the kernels load)
    uint64_t n_selected = 0;
    for (uint64_t w = 0; w < wv; w++) {
        sel[w] &= valid_mask(w, g->n_cols);
        n_selected += (uint64_t)__builtin_popcountll(sel[w]);
    }
    g->n_selected = (uint32_t)n_selected;
    int rc = g->planes.reserve(g->plane_bytes());
    if (rc == BIGSI_OK) rc = g->used.reserve((size_t)2 * n_variants * 4);
    if (rc == BIGSI_OK) rc = g->sel.reserve((size_t)wv * 8);
    if (rc == BIGSI_OK) rc = g->variant_counts.reserve((size_t)n_variants * 16);
    if (rc == BIGSI_OK) rc = g->sample_counts.reserve((size_t)wv * 64 * 8);
    if (rc == BIGSI_OK) {
        hipError_t e = hipMemcpyAsync(g->sel.p, sel.data(), (size_t)wv * 8, hipMemcpyHostToDevice, ix->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(ix->stream);      // (a pageable source that dies with this call)
        if (e != hipSuccess) rc = fail(BIGSI_ERR_HIP, "uploading the column selection: %s", hipGetErrorString(e));
    }
    if (rc == BIGSI_OK) rc = genotype_zero(g, ix->stream);
    if (rc != BIGSI_OK) { bigsi_hip_genotype_destroy(g); return rc; }
    *out = g;
    return BIGSI_OK;
}

extern "C" int bigsi_hip_genotype_destroy(bigsi_hip_genotype *g)
{
    BusyGuard busy_guard_(g ? g->ix : nullptr, /*wait=*/true);
    if (!g) return BIGSI_OK;
    hipError_t e = hipSetDevice(g->ix->device);
    if (g->last) { e = hipEventSynchronize(g->last); e = hipEventDestroy(g->last); }
    for (int s = 0; s < 2; s++) {
        if (g->pin_ev[s]) { e = hipEventSynchronize(g->pin_ev[s]); e = hipEventDestroy(g->pin_ev[s]); }
        if (g->pin[s]) e = hipHostFree(g->pin[s]);
        g->d_allele[s].release();
    }
    (void)e;
    g->planes.release(); g->used.release(); g->sel.release(); g->variant_counts.release(); g->sample_counts.release();
    delete g;
    return BIGSI_OK;
}

extern "C" int bigsi_hip_genotype_reset(bigsi_hip_genotype *g)
{
    BIGSI_ENTER(g ? g->ix : nullptr);
    if (!g) return fail(BIGSI_ERR_INVALID, "NULL accumulator");
    TRY(genotype_check(g, false));
    TRY(use_device(g->ix));
    hipStream_t st = g->ix->stream;
    TRY(genotype_order(g, st));
    TRY(genotype_zero(g, st));
    g->unusable = false;
    return BIGSI_OK;
}

static int genotype_validate(const bigsi_hip_genotype *g, const uint32_t *allele_of, uint64_t n_entries)
{
    const uint64_t bad = genotype_bad_allele(allele_of, n_entries, g->n_variants);
    if (bad != n_entries)
        return fail(BIGSI_ERR_INVALID, "allele_of[%llu] = %u is neither below 2 x n_variants (%u) nor BIGSI_GENOTYPE_NONE", (unsigned long long)bad, allele_of[bad],
                    2 * g->n_variants);
    return BIGSI_OK;
}

// k_allele_or for a batch that passed check_consumer_batch (its result vectors are then as wide as the planes) and whose validated
// allele_of entries are `allele_of`, and finish_consumer
static int genotype_launch(bigsi_hip_genotype *g, bigsi_hip_batch *b, const uint32_t *allele_of)
{
    bigsi_hip_index *ix = b->ix;
    hipStream_t st = consumer_stream(b);
    const GenotypePlan p = plan_genotype(b->n_seqs, b->wv, g->n_variants);
    if (p.too_large) return fail(BIGSI_ERR_INVALID, "batch too large for one genotype launch (%llu workgroups)", (unsigned long long)p.too_large);
    if (p.grid == 0) return BIGSI_OK;
    const int slot = (int)(g->turn++ & 1u);
    const size_t bytes = (size_t)b->n_seqs * 4;
    if (g->pin_ev[slot]) HIP_TRY(hipEventSynchronize(g->pin_ev[slot]));      // (the upload of two adds ago has left the pinned slot)
    else HIP_TRY(hipEventCreateWithFlags(&g->pin_ev[slot], hipEventDisableTiming));
    if (g->pin_cap[slot] < bytes) {
        if (g->pin[slot]) { HIP_TRY(hipHostFree(g->pin[slot])); g->pin[slot] = nullptr; g->pin_cap[slot] = 0; }
        const size_t want = std::max<size_t>(bytes, (size_t)kTallyChunkSeqs * 4);
        HIP_TRY(hipHostMalloc(&g->pin[slot], want, hipHostMallocDefault));
        g->pin_cap[slot] = want;
    }
    memcpy(g->pin[slot], allele_of, bytes);
    TRY(genotype_order(g, st));                      // (also: the kernel that read this slot's device copy two adds ago is behind us)
    if (g->d_allele[slot].cap < bytes) HIP_TRY(hipStreamSynchronize(st));      // (growing frees the old copy)
    TRY(g->d_allele[slot].reserve(std::max<size_t>(bytes, (size_t)kTallyChunkSeqs * 4)));
    HIP_TRY(hipMemcpyAsync(g->d_allele[slot].p, g->pin[slot], bytes, hipMemcpyHostToDevice, st));
    HIP_TRY(hipEventRecord(g->pin_ev[slot], st));
    EventPair ep{};
    TRY(bigsi_ev_begin(ix, &ep, st));
    hipLaunchKernelGGL(k_allele_or, dim3((unsigned)p.grid), dim3(p.block), 0, st, static_cast<const uint64_t *>(b->bit_vectors()), b->wv_pad, (uint32_t)b->wv,
                       g->n_cols, b->n_seqs, b->num_unique.as<uint32_t>(), g->d_allele[slot].as<uint32_t>(), (uint32_t)p.word_blocks,
                       g->planes.as<unsigned long long>(), g->used.as<uint32_t>());
    HIP_TRY(hipGetLastError());
    TRY(bigsi_ev_end(ix, &ep, ix->ev_cp, st, 1));      // (timed with the compaction it stands in for: bigsi_hip_stats' compact_ms)
    TRY(genotype_mark(g, st));
    return finish_consumer(b, st);
}

extern "C" int bigsi_hip_genotype_add_batch(bigsi_hip_genotype *g, bigsi_hip_batch *b, const uint32_t *allele_of, uint64_t n_entries)
{
    BIGSI_ENTER(g ? g->ix : nullptr);
    if (!g || !b || !allele_of) return fail(BIGSI_ERR_INVALID, "NULL argument");
    TRY(genotype_check(g));
    if (b->ix != g->ix) return fail(BIGSI_ERR_STATE, "the batch belongs to another index than the genotype accumulator");
    TRY(check_consumer_batch(b, kGenotypeConsumer));
    if (n_entries != b->n_seqs)
        return fail(BIGSI_ERR_INVALID, "allele_of has %llu entries, the batch has %u sequences", (unsigned long long)n_entries, b->n_seqs);
    TRY(genotype_validate(g, allele_of, n_entries));
    TRY(use_device(g->ix));
    return genotype_launch(g, b, allele_of);
}

// consume_stream over the index's genotype_ws.  A chunk without a k-mer position adds nothing: used counts only probes with k-mers.
extern "C" int bigsi_hip_genotype_add_stream(bigsi_hip_genotype *g, const char *seqs, const uint64_t *offsets, uint64_t n_seqs, uint32_t k, double threshold,
                                             const uint32_t *allele_of)
{
    BIGSI_ENTER(g ? g->ix : nullptr);
    if (!g || !offsets || !allele_of) return fail(BIGSI_ERR_INVALID, "NULL argument");
    TRY(genotype_check(g));
    TRY(check_stream_args(seqs, offsets, n_seqs, k, threshold));
    TRY(genotype_validate(g, allele_of, n_seqs));
    TRY(use_device(g->ix));
    const int rc = consume_stream(
        g->ix, g->ix->genotype_ws, kGenotypeConsumer, seqs, offsets, n_seqs, k, threshold, [](uint64_t, uint64_t) {},
        [&](bigsi_hip_batch *b, int, uint64_t s0, uint64_t) { return genotype_launch(g, b, allele_of + s0); });
    if (rc != BIGSI_OK) g->unusable = true;
    return rc;
}

extern "C" int bigsi_hip_genotype_fetch(bigsi_hip_genotype *g, uint8_t *ref_planes, uint8_t *alt_planes, uint64_t plane_capacity_bytes,
                                        uint32_t *variant_counts, uint32_t *sample_counts, uint64_t sample_capacity, uint32_t *allele_probes)
{
    BIGSI_ENTER(g ? g->ix : nullptr);
    if (!g || !variant_counts || !sample_counts || !allele_probes) return fail(BIGSI_ERR_INVALID, "NULL argument");
    TRY(genotype_check(g));
    const uint64_t rb = g->row_bytes();
    if ((ref_planes || alt_planes) && plane_capacity_bytes < (uint64_t)g->n_variants * rb)
        return fail(BIGSI_ERR_CAPACITY, "a plane buffer holds %llu bytes, %u variants x %llu bytes needed", (unsigned long long)plane_capacity_bytes,
                    g->n_variants, (unsigned long long)rb);
    if (sample_capacity < g->n_cols)
        return fail(BIGSI_ERR_CAPACITY, "sample_counts holds %llu entries, %llu needed", (unsigned long long)sample_capacity, (unsigned long long)g->n_cols);
    TRY(use_device(g->ix));
    hipStream_t st = g->ix->stream;
    TRY(genotype_order(g, st));
    const GenotypePlan p = plan_genotype(1, g->wv, g->n_variants);
    hipLaunchKernelGGL(k_genotype_variants, dim3((unsigned)p.variants_grid), dim3(p.block), 0, st, g->planes.as<uint64_t>(), g->sel.as<uint64_t>(), (uint32_t)g->wv,
                       g->n_variants, g->n_selected, g->variant_counts.as<uint4>());
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(k_genotype_samples, dim3((unsigned)p.samples_grid), dim3(p.block), 0, st, g->planes.as<uint64_t>(), (uint32_t)g->wv, g->n_variants,
                       g->sample_counts.as<uint2>());
    HIP_TRY(hipGetLastError());
    TRY(genotype_mark(g, st));
    // (downloads into host copies first: a failure half way must not leave a caller's buffer half written)
    std::vector<uint32_t> vc((size_t)g->n_variants * 4), sc((size_t)g->n_cols * 2), ap((size_t)g->n_variants * 2);
    HIP_TRY(hipMemcpyAsync(vc.data(), g->variant_counts.p, vc.size() * 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(sc.data(), g->sample_counts.p, sc.size() * 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(ap.data(), g->used.p, ap.size() * 4, hipMemcpyDeviceToHost, st));
    const uint8_t *dp = static_cast<const uint8_t *>(g->planes.p);
    if (ref_planes) HIP_TRY(hipMemcpy2DAsync(ref_planes, rb, dp, 2 * g->wv * 8, rb, g->n_variants, hipMemcpyDeviceToHost, st));
    if (alt_planes) HIP_TRY(hipMemcpy2DAsync(alt_planes, rb, dp + g->wv * 8, 2 * g->wv * 8, rb, g->n_variants, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    memcpy(variant_counts, vc.data(), vc.size() * 4);
    memcpy(sample_counts, sc.data(), sc.size() * 4);
    memcpy(allele_probes, ap.data(), ap.size() * 4);
    return BIGSI_OK;
}

// Locus typing (include/bigsi_hip_typing.h; k_locus_best + k_locus_counts, launch shapes: plan_typing): the fifth consumer, a
// segmented max with argmax over the result vectors and the counters -- the first whose answer depends on the counter VALUES of
// competing records.  The accumulator owns best[n_loci][wv * 64] (uint64), hits[n_loci][wv * 64] and records[n_loci] (uint32), the
// selection vector sel[wv] (columns & valid_mask, built at create), the two count outputs of a fetch, and two staging slots for the
// labels (pinned host + device; locus_of in the first half of a slot, allele_of in the second): an add copies its entries into the
// slot of its turn and uploads from there, so the caller's arrays are not read after the call returns and no add waits for its own
// kernel.  `last` orders the accumulator with itself, as the tally's does.
static_assert(BIGSI_TYPING_NONE == kTypingNone && BIGSI_TYPING_MAX_ALLELE == kTypingMaxAllele && BIGSI_TYPING_MAX_LOCI == kTypingMaxLoci &&
                  BIGSI_TYPING_CELL_BYTES == kTypingCellBytes,
              "header and planner");
constexpr VectorConsumer kTypingConsumer = {"a typing", "ranks", false};

struct bigsi_hip_typing {
    bigsi_hip_index *ix = nullptr;
    uint64_t n_cols = 0, m = 0, wv = 0;
    uint32_t h = 0, n_loci = 0;
    DevBuf best, hits, records, sel, locus_counts, sample_counts;
    DevBuf d_labels[2];
    void *pin[2] = {nullptr, nullptr};
    size_t pin_cap[2] = {0, 0};
    hipEvent_t pin_ev[2] = {nullptr, nullptr};      // behind the upload out of pin[slot]
    unsigned turn = 0;
    hipEvent_t last = nullptr;
    hipStream_t last_stream = nullptr;
    bool unusable = false;                          // a typing_add_stream failed half way: until typing_reset
    size_t cells() const { return (size_t)n_loci * wv * 64; }
};

static int typing_check(const bigsi_hip_typing *t, bool usable = true)
{
    const bigsi_hip_index *ix = t->ix;
    if (ix->n_cols != t->n_cols || ix->m != t->m || ix->h != t->h)
        return fail(BIGSI_ERR_STATE, "the index has changed since bigsi_hip_typing_create (%llu columns, %llu rows, %u hashes then; %llu, %llu, %u now)",
                    (unsigned long long)t->n_cols, (unsigned long long)t->m, t->h, (unsigned long long)ix->n_cols, (unsigned long long)ix->m, ix->h);
    if (usable && t->unusable)
        return fail(BIGSI_ERR_STATE, "a bigsi_hip_typing_add_stream on this accumulator failed half way: bigsi_hip_typing_reset starts over");
    return BIGSI_OK;
}

// what is queued on `st` next comes after everything queued on behalf of the accumulator so far
static int typing_order(bigsi_hip_typing *t, hipStream_t st)
{
    if (t->last && t->last_stream != st) HIP_TRY(hipStreamWaitEvent(st, t->last, 0));
    return BIGSI_OK;
}

static int typing_mark(bigsi_hip_typing *t, hipStream_t st)
{
    if (!t->last) HIP_TRY(hipEventCreateWithFlags(&t->last, hipEventDisableTiming));
    HIP_TRY(hipEventRecord(t->last, st));
    t->last_stream = st;
    return BIGSI_OK;
}

static int typing_zero(bigsi_hip_typing *t, hipStream_t st)
{
    HIP_TRY(hipMemsetAsync(t->best.p, 0, t->cells() * 8, st));
    HIP_TRY(hipMemsetAsync(t->hits.p, 0, t->cells() * 4, st));
    HIP_TRY(hipMemsetAsync(t->records.p, 0, (size_t)t->n_loci * 4, st));
    return typing_mark(t, st);
}

extern "C" int bigsi_hip_typing_create(bigsi_hip_index *ix, uint32_t n_loci, const uint8_t *columns, bigsi_hip_typing **out)
{
    BIGSI_ENTER(ix);
    if (!ix || !out) return fail(BIGSI_ERR_INVALID, "NULL argument");
    *out = nullptr;
    if (ix->n_cols == 0) return fail(BIGSI_ERR_STATE, "index has no columns");
    const uint64_t wv = ix->wv();
    const TypingPlan p = plan_typing(1, wv, n_loci);
    if (p.bad_loci) return fail(BIGSI_ERR_INVALID, "n_loci must be 1 .. BIGSI_TYPING_MAX_LOCI = %u (got %u)", kTypingMaxLoci, n_loci);
    if (p.too_many_bytes)
        return fail(BIGSI_ERR_NOMEM, "the cells of %u loci over %llu columns take %u x %llu x 64 x 12 bytes, above BIGSI_TYPING_CELL_BYTES = %llu: slice the scheme by locus",
                    n_loci, (unsigned long long)ix->n_cols, n_loci, (unsigned long long)wv, (unsigned long long)kTypingCellBytes);
    if (p.too_large) return fail(BIGSI_ERR_INVALID, "index too wide for one typing launch (%llu workgroups)", (unsigned long long)p.too_large);
    TRY(use_device(ix));
    bigsi_hip_typing *t = new (std::nothrow) bigsi_hip_typing();
    if (!t) return fail(BIGSI_ERR_NOMEM, "host allocation failed");
    t->ix = ix;
    t->n_cols = ix->n_cols; t->m = ix->m; t->h = ix->h; t->wv = wv;
    t->n_loci = n_loci;
    std::vector<uint64_t> sel(wv, columns ? 0ull : ~0ull);
    if (columns) memcpy(sel.data(), columns, (size_t)((t->n_cols + 7) / 8));      // (row format = the little-endian words the kernels load)
    for (uint64_t w = 0; w < wv; w++) sel[w] &= valid_mask(w, t->n_cols);
    int rc = t->best.reserve(t->cells() * 8);
    if (rc == BIGSI_OK) rc = t->hits.reserve(t->cells() * 4);
    if (rc == BIGSI_OK) rc = t->records.reserve((size_t)n_loci * 4);
    if (rc == BIGSI_OK) rc = t->sel.reserve((size_t)wv * 8);
    if (rc == BIGSI_OK) rc = t->locus_counts.reserve((size_t)n_loci * 12);
    if (rc == BIGSI_OK) rc = t->sample_counts.reserve((size_t)wv * 64 * 8);
    if (rc == BIGSI_OK) {
        hipError_t e = hipMemcpyAsync(t->sel.p, sel.data(), (size_t)wv * 8, hipMemcpyHostToDevice, ix->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(ix->stream);      // (a pageable source that dies with this call)
        if (e != hipSuccess) rc = fail(BIGSI_ERR_HIP, "uploading the column selection: %s", hipGetErrorString(e));
    }
    if (rc == BIGSI_OK) rc = typing_zero(t, ix->stream);
    if (rc != BIGSI_OK) { bigsi_hip_typing_destroy(t); return rc; }
    *out = t;
    return BIGSI_OK;
}

extern "C" int bigsi_hip_typing_destroy(bigsi_hip_typing *t)
{
    BusyGuard busy_guard_(t ? t->ix : nullptr, /*wait=*/true);
    if (!t) return BIGSI_OK;
    hipError_t e = hipSetDevice(t->ix->device);
    if (t->last) { e = hipEventSynchronize(t->last); e = hipEventDestroy(t->last); }
    for (int s = 0; s < 2; s++) {
        if (t->pin_ev[s]) { e = hipEventSynchronize(t->pin_ev[s]); e = hipEventDestroy(t->pin_ev[s]); }
        if (t->pin[s]) e = hipHostFree(t->pin[s]);
        t->d_labels[s].release();
    }
    (void)e;
    t->best.release(); t->hits.release(); t->records.release(); t->sel.release(); t->locus_counts.release(); t->sample_counts.release();
    delete t;
    return BIGSI_OK;
}

extern "C" int bigsi_hip_typing_reset(bigsi_hip_typing *t)
{
    BIGSI_ENTER(t ? t->ix : nullptr);
    if (!t) return fail(BIGSI_ERR_INVALID, "NULL accumulator");
    TRY(typing_check(t, false));
    TRY(use_device(t->ix));
    hipStream_t st = t->ix->stream;
    TRY(typing_order(t, st));
    TRY(typing_zero(t, st));
    t->unusable = false;
    return BIGSI_OK;
}

static int typing_validate(const bigsi_hip_typing *t, const uint32_t *locus_of, const uint32_t *allele_of, uint64_t n_entries)
{
    const uint64_t bad = typing_bad_label(locus_of, allele_of, n_entries, t->n_loci);
    if (bad == n_entries) return BIGSI_OK;
    if (locus_of[bad] >= t->n_loci)
        return fail(BIGSI_ERR_INVALID, "locus_of[%llu] = %u is neither below n_loci (%u) nor BIGSI_TYPING_NONE", (unsigned long long)bad, locus_of[bad], t->n_loci);
    return fail(BIGSI_ERR_INVALID, "allele_of[%llu] = %u is above BIGSI_TYPING_MAX_ALLELE = %u", (unsigned long long)bad, allele_of[bad], kTypingMaxAllele);
}

// k_locus_best for a batch that passed check_consumer_batch (its result vectors are then as wide as the cells' rows) and whose
// validated labels are `locus_of` and `allele_of`, and finish_consumer
static int typing_launch(bigsi_hip_typing *t, bigsi_hip_batch *b, const uint32_t *locus_of, const uint32_t *allele_of)
{
    bigsi_hip_index *ix = b->ix;
    hipStream_t st = consumer_stream(b);
    const TypingPlan p = plan_typing(b->n_seqs, b->wv, t->n_loci);
    if (p.too_large) return fail(BIGSI_ERR_INVALID, "batch too large for one typing launch (%llu workgroups)", (unsigned long long)p.too_large);
    if (p.grid == 0) return BIGSI_OK;
    const int slot = (int)(t->turn++ & 1u);
    const size_t half = (size_t)b->n_seqs * 4, bytes = 2 * half;
    if (t->pin_ev[slot]) HIP_TRY(hipEventSynchronize(t->pin_ev[slot]));      // (the upload of two adds ago has left the pinned slot)
    else HIP_TRY(hipEventCreateWithFlags(&t->pin_ev[slot], hipEventDisableTiming));
    if (t->pin_cap[slot] < bytes) {
        if (t->pin[slot]) { HIP_TRY(hipHostFree(t->pin[slot])); t->pin[slot] = nullptr; t->pin_cap[slot] = 0; }
        const size_t want = std::max<size_t>(bytes, (size_t)kTallyChunkSeqs * 8);
        HIP_TRY(hipHostMalloc(&t->pin[slot], want, hipHostMallocDefault));
        t->pin_cap[slot] = want;
    }
    memcpy(t->pin[slot], locus_of, half);
    memcpy(static_cast<char *>(t->pin[slot]) + half, allele_of, half);
    TRY(typing_order(t, st));                        // (also: the kernel that read this slot's device copy two adds ago is behind us)
    if (t->d_labels[slot].cap < bytes) HIP_TRY(hipStreamSynchronize(st));      // (growing frees the old copy)
    TRY(t->d_labels[slot].reserve(std::max<size_t>(bytes, (size_t)kTallyChunkSeqs * 8)));
    HIP_TRY(hipMemcpyAsync(t->d_labels[slot].p, t->pin[slot], bytes, hipMemcpyHostToDevice, st));
    HIP_TRY(hipEventRecord(t->pin_ev[slot], st));
    const uint32_t *d_locus = t->d_labels[slot].as<uint32_t>(), *d_allele = d_locus + b->n_seqs;
    const uint64_t *bm = static_cast<const uint64_t *>(b->bit_vectors());
    const uint64_t cstride = b->wv_pad * 64;
    EventPair ep{};
    TRY(bigsi_ev_begin(ix, &ep, st));
    with_counters(b, [&](auto exact, const auto *cnt) {
        using CountT = std::remove_const_t<std::remove_pointer_t<decltype(cnt)>>;
        hipLaunchKernelGGL((k_locus_best<CountT, decltype(exact)::value>), dim3((unsigned)p.grid), dim3(p.block), 0, st, bm, b->wv_pad, (uint32_t)b->wv, b->n_seqs,
                           b->num_unique.as<uint32_t>(), cnt, cstride, d_locus, d_allele, t->sel.as<uint64_t>(), (uint32_t)p.word_groups,
                           t->best.as<unsigned long long>(), t->hits.as<uint32_t>(), t->records.as<uint32_t>());
    });
    HIP_TRY(hipGetLastError());
    TRY(bigsi_ev_end(ix, &ep, ix->ev_cp, st, 1));      // (timed with the compaction it stands in for: bigsi_hip_stats' compact_ms)
    TRY(typing_mark(t, st));
    return finish_consumer(b, st);
}

extern "C" int bigsi_hip_typing_add_batch(bigsi_hip_typing *t, bigsi_hip_batch *b, const uint32_t *locus_of, const uint32_t *allele_of, uint64_t n_entries)
{
    BIGSI_ENTER(t ? t->ix : nullptr);
    if (!t || !b || !locus_of || !allele_of) return fail(BIGSI_ERR_INVALID, "NULL argument");
    TRY(typing_check(t));
    if (b->ix != t->ix) return fail(BIGSI_ERR_STATE, "the batch belongs to another index than the typing accumulator");
    TRY(check_consumer_batch(b, kTypingConsumer));
    if (n_entries != b->n_seqs)
        return fail(BIGSI_ERR_INVALID, "locus_of and allele_of have %llu entries, the batch has %u sequences", (unsigned long long)n_entries, b->n_seqs);
    TRY(typing_validate(t, locus_of, allele_of, n_entries));
    TRY(use_device(t->ix));
    return typing_launch(t, b, locus_of, allele_of);
}

// consume_stream over the index's typing_ws.  A chunk without a k-mer position adds nothing: records counts only records with k-mers.
extern "C" int bigsi_hip_typing_add_stream(bigsi_hip_typing *t, const char *seqs, const uint64_t *offsets, uint64_t n_seqs, uint32_t k, double threshold,
                                           const uint32_t *locus_of, const uint32_t *allele_of)
{
    BIGSI_ENTER(t ? t->ix : nullptr);
    if (!t || !offsets || !locus_of || !allele_of) return fail(BIGSI_ERR_INVALID, "NULL argument");
    TRY(typing_check(t));
    TRY(check_stream_args(seqs, offsets, n_seqs, k, threshold));
    TRY(typing_validate(t, locus_of, allele_of, n_seqs));
    TRY(use_device(t->ix));
    const int rc = consume_stream(
        t->ix, t->ix->typing_ws, kTypingConsumer, seqs, offsets, n_seqs, k, threshold, [](uint64_t, uint64_t) {},
        [&](bigsi_hip_batch *b, int, uint64_t s0, uint64_t) { return typing_launch(t, b, locus_of + s0, allele_of + s0); });
    if (rc != BIGSI_OK) t->unusable = true;
    return rc;
}

extern "C" int bigsi_hip_typing_fetch(bigsi_hip_typing *t, uint64_t *best, uint32_t *hits, uint64_t cell_capacity, uint32_t *locus_counts,
                                      uint32_t *sample_counts, uint64_t sample_capacity, uint32_t *records)
{
    BIGSI_ENTER(t ? t->ix : nullptr);
    if (!t || !locus_counts || !sample_counts || !records) return fail(BIGSI_ERR_INVALID, "NULL argument");
    TRY(typing_check(t));
    if ((best || hits) && cell_capacity < (uint64_t)t->n_loci * t->n_cols)
        return fail(BIGSI_ERR_CAPACITY, "a cell buffer holds %llu entries, %u loci x %llu columns needed", (unsigned long long)cell_capacity, t->n_loci,
                    (unsigned long long)t->n_cols);
    if (sample_capacity < t->n_cols)
        return fail(BIGSI_ERR_CAPACITY, "sample_counts holds %llu entries, %llu needed", (unsigned long long)sample_capacity, (unsigned long long)t->n_cols);
    TRY(use_device(t->ix));
    hipStream_t st = t->ix->stream;
    TRY(typing_order(t, st));
    const TypingPlan p = plan_typing(1, t->wv, t->n_loci);
    hipLaunchKernelGGL(k_locus_counts, dim3((unsigned)p.counts_grid), dim3(p.block), 0, st, t->best.as<uint64_t>(), t->hits.as<uint32_t>(), (uint32_t)t->wv, t->n_loci,
                       (uint32_t)p.loci_grid, t->locus_counts.as<uint32_t>(), t->sample_counts.as<uint2>());
    HIP_TRY(hipGetLastError());
    TRY(typing_mark(t, st));
    // (downloads into host copies first: a failure half way must not leave a caller's buffer half written)
    std::vector<uint32_t> lc((size_t)t->n_loci * 3), sc((size_t)t->n_cols * 2), rec((size_t)t->n_loci);
    HIP_TRY(hipMemcpyAsync(lc.data(), t->locus_counts.p, lc.size() * 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(sc.data(), t->sample_counts.p, sc.size() * 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(rec.data(), t->records.p, rec.size() * 4, hipMemcpyDeviceToHost, st));
    const size_t row = (size_t)t->wv * 64;      // (cell 64 w + lane of a row is column 64 w + lane: a row's first num_cols cells are the columns)
    if (best) HIP_TRY(hipMemcpy2DAsync(best, t->n_cols * 8, t->best.p, row * 8, t->n_cols * 8, t->n_loci, hipMemcpyDeviceToHost, st));
    if (hits) HIP_TRY(hipMemcpy2DAsync(hits, t->n_cols * 4, t->hits.p, row * 4, t->n_cols * 4, t->n_loci, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    memcpy(locus_counts, lc.data(), lc.size() * 4);
    memcpy(sample_counts, sc.data(), sc.size() * 4);
    memcpy(records, rec.data(), rec.size() * 4);
    return BIGSI_OK;
}

// K5 at scale: the presence strings of all hits of the batch (see k_presence_bits).  The host sorts each sequence's hits by
// colour and groups them into 128-column word pairs (a few microseconds per thousand hits); the device does the rest.
// K5 / K6 for the hits of a batch, in two halves so that a serving loop can overlap them with other work:
//   presence_begin  host: string / bit offsets, per-sequence colour order, word pairs -> pinned staging; device (asynchronous):
//                   upload, k_presence_bits, then either the ASCII strings (k_presence_expand*, K5) or the packed presence bits
//                   + score records (k_presence_score, K6), download into pinned staging, completion event.
//   presence_end    waits for that event and copies the staged results into the caller's buffers.
// The kernels go to the library's score stream (highest priority: the host is waiting for them while the next batch's row-AND
// kernel fills the device) or, BIGSI_SCORE_ORDERED, to the index stream behind whatever is already queued there: alone on
// the device they take a tenth of the time they take beside a row-AND kernel, and a loop three batches deep never waits for
// them (bench workload c5).
static_assert(sizeof(bigsi_hip_hit_score) == sizeof(bigsi_score::HitScore) && sizeof(bigsi_hip_hit_score) == 64, "score record layout");

static int pinned_reserve(void **p, size_t *cap, size_t bytes)
{
    if (bytes <= *cap) return BIGSI_OK;
    if (*p) { hipError_t e = hipHostFree(*p); (void)e; *p = nullptr; *cap = 0; }
    const size_t want = std::max<size_t>(bytes + bytes / 4, 4096);
    HIP_TRY(hipHostMalloc(p, want, hipHostMallocCoherent | hipHostMallocMapped));      // (kernels write results / read small inputs here directly)
    *cap = want;
    return BIGSI_OK;
}

static int presence_begin(bigsi_hip_batch *b, const uint64_t *hit_offsets, const uint32_t *colours, const uint32_t *counts, bool packed,
                          bool ordered, uint64_t out_capacity, bool check_capacity, uint64_t *string_offsets)
{
    TRY(need_run(b));
    if (!hit_offsets || !string_offsets) return fail(BIGSI_ERR_INVALID, "NULL argument");
    PresJob &job = b->job;
    if (job.pending) return fail(BIGSI_ERR_STATE, "a score / presence request of this batch is still pending (call the matching _end)");
    bigsi_hip_index *ix = b->ix;
    const uint32_t nq = b->n_seqs;
    const uint64_t n_hits = hit_offsets[nq] - hit_offsets[0], h0 = hit_offsets[0];
    if (n_hits && !colours) return fail(BIGSI_ERR_INVALID, "colours is NULL");
    if (n_hits > 0xFFFFFFF0ull) return fail(BIGSI_ERR_INVALID, "too many hits for one call");
    TRY(host_counts(b));
    hipStream_t ps = ix->stream;
    if (!ordered) TRY(score_stream(ix, &ps));
    // host side: string offsets, per-sequence colour order, word pairs
    std::vector<uint32_t> &hit_seq = job.hit_seq, &hit_q = job.hit_q, &perm = job.perm, &order = job.order;      // hit_seq: k-mers of the hit's sequence (its string length); hit_q: which sequence
    std::vector<uint64_t> &hit_pos0 = job.hit_pos0;
    std::vector<PresencePair> pairs;
    std::vector<PresenceWave> waves;          // (k_presence_bits: a wavefront = up to 64 pairs of one query)
    hit_seq.resize(n_hits); hit_q.resize(n_hits); perm.resize(n_hits); hit_pos0.resize(n_hits);
    pairs.clear();
    for (uint64_t t = 0; t < n_hits; t++) perm[t] = (uint32_t)t;
    uint64_t str = 0, alg = 0;
    uint32_t max_u = 0, max_n = 0;
    for (uint32_t q = 0; q < nq; q++) {
        if (hit_offsets[q + 1] < hit_offsets[q]) return fail(BIGSI_ERR_INVALID, "hit_offsets must be non-decreasing");
        const uint64_t lo = hit_offsets[q] - h0, hi = hit_offsets[q + 1] - h0;
        for (uint64_t t = lo; t < hi; t++) {
            if (colours[h0 + t] >= ix->n_cols) return fail(BIGSI_ERR_RANGE, "colour %u >= num_cols", colours[h0 + t]);
            hit_seq[t] = b->h_num_kmers[q];
            hit_q[t] = q;
            hit_pos0[t] = b->pos_off[q];
            string_offsets[t] = str;
            // every string starts on a 16-byte boundary (16-character stores); packed: whole 8-byte words
            str += packed ? round_up(b->h_num_kmers[q], 64) / 8 : round_up(b->h_num_kmers[q], 16);
        }
        if (hi == lo || b->h_num_kmers[q] == 0) continue;
        const size_t first_pair = pairs.size();
        // the hit lists fetch_hits returns are in colour order already: sort only what is not
        bool sorted = true;
        for (uint64_t t = lo + 1; t < hi && sorted; t++) sorted = colours[h0 + t - 1] < colours[h0 + t];
        if (!sorted) {
            order.resize(hi - lo);
            for (uint64_t t = lo; t < hi; t++) order[t - lo] = (uint32_t)t;
            std::sort(order.begin(), order.end(), [&](uint32_t x, uint32_t y) { return colours[h0 + x] < colours[h0 + y]; });
        }
        uint64_t words = 0, last_word = ~0ull;
        for (uint64_t r = 0; r < hi - lo; r++) {
            const uint32_t src = sorted ? (uint32_t)(lo + r) : order[r];
            const uint32_t c = colours[h0 + src];
            if (r && c == colours[h0 + (sorted ? (uint32_t)(lo + r - 1) : order[r - 1])])
                return fail(BIGSI_ERR_INVALID, "colour %u listed twice for sequence %u", c, q);
            const uint32_t wp = c >> 7;
            if (pairs.size() == first_pair || pairs.back().wpair != wp) pairs.push_back(PresencePair{wp, (uint32_t)(lo + r), 0ull, 0ull, q, 0u});
            const uint64_t bit = 1ull << bit_of_col(c & 63u);
            if (c & 64u) pairs.back().mask_hi |= bit;
            else pairs.back().mask_lo |= bit;
            perm[lo + r] = src;
            if ((uint64_t)(c >> 6) != last_word) { words++; last_word = c >> 6; }
        }
        for (size_t f = first_pair; f < pairs.size(); f += 64) waves.push_back(PresenceWave{(uint32_t)f, (uint32_t)std::min<size_t>(64, pairs.size() - f)});
        max_u = std::max(max_u, b->h_num_unique[q]);
        max_n = std::max(max_n, b->h_num_kmers[q]);
        alg += (uint64_t)b->h_num_unique[q] * b->run_h * words * 8 +
               (hi - lo) * (packed ? round_up(b->h_num_kmers[q], 64) / 8 + sizeof(bigsi_hip_hit_score) : (uint64_t)b->h_num_kmers[q]);
    }
    string_offsets[n_hits] = str;
    if (check_capacity && str > out_capacity)
        return fail(BIGSI_ERR_CAPACITY, "%s buffer holds %llu bytes, %llu needed", packed ? "bit" : "string", (unsigned long long)out_capacity, (unsigned long long)str);
    job.packed = packed;
    job.n_hits = n_hits;
    job.str = str;
    job.o_scores = round_up(str, 256);
    job.device_work = false;
    job.pending = true;
    if (n_hits == 0 || str == 0) return BIGSI_OK;          // (hits of sequences without k-mers: nothing to extract, all-zero records)
    if (b->run_h != ix->h) { job.pending = false; return fail(BIGSI_ERR_STATE, "num_hashes changed since the batch was run"); }
    job.pending = false;                                   // (set again once everything is enqueued)
    // device input: [str_off | hit_seq | perm | hit_pos0 | pairs | hit_q | found | unique] in one upload from pinned memory
    const size_t o_str = 0, o_seq = round_up(o_str + (n_hits + 1) * 8, 256);
    const size_t o_perm = round_up(o_seq + n_hits * 4, 256), o_pos0 = round_up(o_perm + n_hits * 4, 256), o_pairs = round_up(o_pos0 + n_hits * 8, 256);
    const size_t o_waves = round_up(o_pairs + pairs.size() * sizeof(PresencePair), 256);
    const size_t o_q = round_up(o_waves + waves.size() * sizeof(PresenceWave), 256), o_hoff = round_up(o_q + n_hits * 4, 256);
    // (K6) per rank: k-mers the hit found, unique k-mers of its sequence
    const size_t o_found = round_up(o_hoff + (nq + 1) * 8ull, 256), o_uniq = round_up(o_found + (packed ? n_hits * 4 : 0), 256);
    const size_t in_bytes = packed ? o_uniq + n_hits * 4 : o_hoff + (nq + 1) * 8ull;
    TRY(pinned_reserve(&job.h_in, &job.h_in_cap, in_bytes));
    uint8_t *stage = static_cast<uint8_t *>(job.h_in);
    // the device works in rank order (each sequence's hits by colour): string offset of the hit with that rank; the other per-hit
    // values (k-mers, map start, sequence) are the same for all hits of a sequence, whose hits keep their index range
    for (uint64_t r = 0; r < n_hits; r++) reinterpret_cast<uint64_t *>(stage + o_str)[r] = string_offsets[perm[r]];
    memcpy(stage + o_seq, hit_seq.data(), n_hits * 4);
    memcpy(stage + o_perm, perm.data(), n_hits * 4);
    memcpy(stage + o_pos0, hit_pos0.data(), n_hits * 8);
    memcpy(stage + o_pairs, pairs.data(), pairs.size() * sizeof(PresencePair));
    memcpy(stage + o_waves, waves.data(), waves.size() * sizeof(PresenceWave));
    memcpy(stage + o_q, hit_q.data(), n_hits * 4);
    for (uint32_t q = 0; q <= nq; q++) reinterpret_cast<uint64_t *>(stage + o_hoff)[q] = hit_offsets[q] - h0;
    if (packed)
        for (uint64_t r = 0; r < n_hits; r++) {
            const uint32_t u = b->h_num_unique[hit_q[r]];
            reinterpret_cast<uint32_t *>(stage + o_uniq)[r] = u;
            reinterpret_cast<uint32_t *>(stage + o_found)[r] = counts ? counts[h0 + perm[r]] : u;
        }
    const uint32_t n_chunks = (uint32_t)ceil_div(std::max<uint32_t>(max_u, 1), 16);
    const size_t out_bytes = packed ? job.o_scores + n_hits * sizeof(bigsi_hip_hit_score) : str;
    TRY(pinned_reserve(&job.h_out, &job.h_out_cap, out_bytes));
    TRY(b->pres_in.reserve(in_bytes));
    TRY(b->pres_bits.reserve((size_t)round_up(n_hits, 32) * n_chunks * 2 + 16));
    TRY(b->pres_out.reserve(out_bytes));
    const uint64_t max_pieces = (b->total_pos >> 4) + nq + 1;      // marks | list of unmarked pieces | their number
    TRY(b->pres_desc.reserve(round_up(max_pieces * 4, 256) + max_pieces * 8 + 256));
    uint32_t *d_marks = b->pres_desc.as<uint32_t>();
    uint2 *d_listed = reinterpret_cast<uint2 *>(b->pres_desc.as<uint8_t>() + round_up(max_pieces * 4, 256));
    uint32_t *d_listed_n = reinterpret_cast<uint32_t *>(b->pres_desc.as<uint8_t>() + round_up(max_pieces * 4, 256) + max_pieces * 8);
    if (!job.done) HIP_TRY(hipEventCreateWithFlags(&job.done, hipEventDisableTiming));
    b->idle = false;
    if (ps == ix->sc_stream) ix->sc_pending = true;      // from here on something of this index may be queued there
    HIP_TRY(hipMemcpyAsync(b->pres_in.p, stage, in_bytes, hipMemcpyHostToDevice, ps));
    const uint8_t *din = b->pres_in.as<uint8_t>();
    EventPair ep{};
    TRY(ev_begin(ix, &ep, ps));
    if (b->marks_of_run != b->run_serial || b->marks_at != b->pres_desc.p) {
        // the piece marks depend on K1's position -> unique k-mer map alone: once per run of the batch, not once per call
        HIP_TRY(hipMemsetAsync(d_listed_n, 0, 4, ps));
        hipLaunchKernelGGL(k_presence_pieces, dim3(nq), dim3(kBlock), 0, ps, b->pos_unique.as<uint32_t>(), b->d_pos_off.as<uint64_t>(),
                           b->num_kmers.as<uint32_t>(), d_marks, d_listed_n, d_listed);
        b->marks_of_run = b->run_serial;
        b->marks_at = b->pres_desc.p;
    }
    const dim3 grid_a((unsigned)ceil_div(std::max<uint64_t>(waves.size(), 1), kBlock / 64), (unsigned)ceil_div(std::max<uint32_t>(max_u, 1), 16), 1);
#define BIGSI_PRESENCE_ARGS                                                                                                        \
    grid_a, dim3(kBlock), 0, ps, ix->d_index, ix->stride_words, b->rows.as<uint64_t>(), b->d_pos_off.as<uint64_t>(),            \
        b->num_unique.as<uint32_t>(), ix->h, (uint32_t)waves.size(), (const PresenceWave *)(din + o_waves), (const PresencePair *)(din + o_pairs),   \
        b->pres_bits.as<uint16_t>(), n_chunks
#define COMMA ,
#define BIGSI_PRESENCE(H) hipLaunchKernelGGL((k_presence_bits<H COMMA 2>), BIGSI_PRESENCE_ARGS)
    if (!waves.empty()) switch (ix->h) {
    case 1: BIGSI_PRESENCE(1); break;
    case 2: BIGSI_PRESENCE(2); break;
    case 3: BIGSI_PRESENCE(3); break;
    case 4: BIGSI_PRESENCE(4); break;
    case 5: BIGSI_PRESENCE(5); break;
    default: BIGSI_PRESENCE(0); break;
    }
#undef BIGSI_PRESENCE
#undef BIGSI_PRESENCE_ARGS
#undef COMMA
    HIP_TRY(hipGetLastError());
    if (packed) {
        // K6: position-ordered bits of every hit and its score record (written at the hit's place in the caller's order)
        hipLaunchKernelGGL(k_presence_score, dim3((unsigned)ceil_div(n_hits, kBlock)), dim3(kBlock), 0, ps, b->pres_bits.as<uint16_t>(), n_chunks, n_hits,
                           (const uint32_t *)(din + o_seq), (const uint64_t *)(din + o_pos0), (const uint32_t *)(din + o_q), d_marks,
                           b->pos_unique.as<uint32_t>(), (const uint64_t *)(din + o_str), b->pres_out.as<uint8_t>(),
                           (const uint32_t *)(din + o_found), (const uint32_t *)(din + o_uniq), (const uint32_t *)(din + o_perm),
                           reinterpret_cast<bigsi_score::HitScore *>(b->pres_out.as<uint8_t>() + job.o_scores));
    } else {
        const uint32_t pieces = (uint32_t)pow2_at_least(ceil_div(std::max<uint32_t>(max_n, 1), 16));      // power of two: shifts, not divisions
        const uint64_t groups = ceil_div(n_hits, kPresenceHits * kPresenceRounds), blocks = ceil_div(groups * pieces, kBlock);
        if (blocks > 0x7FFFFFFFull || groups > 0x7FFFFFFFull)
            return fail(BIGSI_ERR_INVALID, "presence request too large for one launch");
#define BIGSI_EXPAND_ARGS                                                                                                          \
    dim3((unsigned)blocks), dim3(kBlock), 0, ps, b->pres_bits.as<uint16_t>(), n_chunks, n_hits, pieces,                          \
        (const uint32_t *)(din + o_seq), (const uint64_t *)(din + o_pos0), (const uint64_t *)(din + o_str), b->pres_out.as<uint8_t>(),    \
        (const uint32_t *)(din + o_q), d_marks
        if (pieces >= 64) hipLaunchKernelGGL(k_presence_expand<true>, BIGSI_EXPAND_ARGS);
        else hipLaunchKernelGGL(k_presence_expand<false>, BIGSI_EXPAND_ARGS);
        hipLaunchKernelGGL(k_presence_expand_listed, dim3(1024), dim3(kBlock), 0, ps, b->pres_bits.as<uint16_t>(), n_chunks, d_listed_n, d_listed,
                           (const uint64_t *)(din + o_hoff), b->d_pos_off.as<uint64_t>(), b->num_kmers.as<uint32_t>(), b->pos_unique.as<uint32_t>(),
                           (const uint64_t *)(din + o_str), b->pres_out.as<uint8_t>());
#undef BIGSI_EXPAND_ARGS
    }
    HIP_TRY(hipGetLastError());
    TRY(ev_end(ix, &ep, ix->ev_pr, ps));
    if (ep.a) ix->presence_bytes += alg;
    // one download: [strings or bits | (score records)] are contiguous in pres_out
    HIP_TRY(hipMemcpyAsync(job.h_out, b->pres_out.p, out_bytes, hipMemcpyDeviceToHost, ps));
    HIP_TRY(hipEventRecord(job.done, ps));
    if (ps == ix->sc_stream) ix->sc_pending = true;
    job.device_work = true;
    job.pending = true;
    return BIGSI_OK;
}

static int presence_end(bigsi_hip_batch *b, uint8_t *out, uint64_t out_capacity, bigsi_hip_hit_score *scores)
{
    if (!b) return fail(BIGSI_ERR_INVALID, "NULL batch");
    PresJob &job = b->job;
    if (!job.pending) return fail(BIGSI_ERR_STATE, "no score / presence request of this batch is pending");
    TRY(use_device(b->ix));
    // arguments first: a call that fails on them leaves the request pending (its results stay staged in job.h_out), so the
    // caller can repeat _end with a larger buffer
    if (job.packed && !scores) return fail(BIGSI_ERR_INVALID, "scores is NULL");
    if (job.str > out_capacity)
        return fail(BIGSI_ERR_CAPACITY, "%s buffer holds %llu bytes, %llu needed", job.packed ? "bit" : "string", (unsigned long long)out_capacity, (unsigned long long)job.str);
    if (job.n_hits && job.device_work && !out) return fail(BIGSI_ERR_INVALID, "out is NULL");
    if (job.device_work) HIP_TRY(hipEventSynchronize(job.done));
    job.pending = false;
    if (job.n_hits == 0) return BIGSI_OK;
    if (!job.device_work) {
        if (job.packed) memset(scores, 0, job.n_hits * sizeof(bigsi_hip_hit_score));
        return BIGSI_OK;
    }
    memcpy(out, job.h_out, job.str);
    if (job.packed) memcpy(scores, static_cast<const uint8_t *>(job.h_out) + job.o_scores, job.n_hits * sizeof(bigsi_hip_hit_score));
    return BIGSI_OK;
}

extern "C" int bigsi_hip_batch_presence_hits(bigsi_hip_batch *b, const uint64_t *hit_offsets, const uint32_t *colours, uint8_t *out,
                                             uint64_t out_capacity, uint64_t *string_offsets)
{
    BIGSI_ENTER(b ? b->ix : nullptr);
    TRY(presence_begin(b, hit_offsets, colours, nullptr, false, false, out_capacity, true, string_offsets));
    return presence_end(b, out, out_capacity, nullptr);
}

extern "C" int bigsi_hip_batch_score_hits(bigsi_hip_batch *b, const uint64_t *hit_offsets, const uint32_t *colours, const uint32_t *counts,
                                          uint8_t *bits, uint64_t bits_capacity, uint64_t *bit_offsets, bigsi_hip_hit_score *scores)
{
    BIGSI_ENTER(b ? b->ix : nullptr);
    if (!scores) return fail(BIGSI_ERR_INVALID, "scores is NULL");
    TRY(presence_begin(b, hit_offsets, colours, counts, true, false, bits_capacity, true, bit_offsets));
    return presence_end(b, bits, bits_capacity, scores);
}

extern "C" int bigsi_hip_batch_score_hits_begin(bigsi_hip_batch *b, const uint64_t *hit_offsets, const uint32_t *colours, const uint32_t *counts,
                                                uint32_t flags, uint64_t *bit_offsets)
{
    BIGSI_ENTER(b ? b->ix : nullptr);
    return presence_begin(b, hit_offsets, colours, counts, true, (flags & BIGSI_SCORE_ORDERED) != 0, 0, false, bit_offsets);
}

extern "C" int bigsi_hip_batch_score_hits_end(bigsi_hip_batch *b, uint8_t *bits, uint64_t bits_capacity, bigsi_hip_hit_score *scores)
{
    BIGSI_ENTER(b ? b->ix : nullptr);
    if (!scores) return fail(BIGSI_ERR_INVALID, "scores is NULL");
    return presence_end(b, bits, bits_capacity, scores);
}

// Scorer.score for presence strings the caller already holds as bits: no index involved (one upload, K6's scoring kernel,
// one download).
extern "C" int bigsi_hip_score_presence(int device, const uint8_t *bits, const uint64_t *bit_offsets, const uint32_t *num_kmers,
                                        const uint32_t *found, const uint32_t *unique, uint64_t n, bigsi_hip_hit_score *scores)
{
    if (n == 0) return BIGSI_OK;
    if (!bits || !bit_offsets || !num_kmers || !scores) return fail(BIGSI_ERR_INVALID, "NULL argument");
    if (n > 0x7FFFFFFFull * kBlock) return fail(BIGSI_ERR_INVALID, "too many strings for one call");
    uint64_t end = 0;
    for (uint64_t t = 0; t < n; t++) {
        if (bit_offsets[t] & 7u) return fail(BIGSI_ERR_INVALID, "bit_offsets[%llu] is not a multiple of 8", (unsigned long long)t);
        end = std::max(end, bit_offsets[t] + round_up(num_kmers[t], 64) / 8);
    }
    HIP_TRY(hipSetDevice(device));
    const size_t o_off = round_up(end, 256), o_n = round_up(o_off + n * 8, 256), o_f = round_up(o_n + n * 4, 256), o_u = round_up(o_f + n * 4, 256);
    const size_t o_out = round_up(o_u + n * 4, 256), total = o_out + n * sizeof(bigsi_hip_hit_score);
    std::vector<uint8_t> stage(o_out, 0);
    memcpy(stage.data(), bits, end);
    memcpy(stage.data() + o_off, bit_offsets, n * 8);
    memcpy(stage.data() + o_n, num_kmers, n * 4);
    if (found) memcpy(stage.data() + o_f, found, n * 4);
    if (unique) memcpy(stage.data() + o_u, unique, n * 4);
    uint8_t *d = nullptr;
    HIP_TRY(hipMalloc((void **)&d, total));
    hipError_t e = hipMemcpy(d, stage.data(), o_out, hipMemcpyHostToDevice);
    if (e == hipSuccess) {
        hipLaunchKernelGGL(k_score_packed, dim3((unsigned)ceil_div(n, kBlock)), dim3(kBlock), 0, 0, d, (const uint64_t *)(d + o_off), n,
                           (const uint32_t *)(d + o_n), found ? (const uint32_t *)(d + o_f) : nullptr, unique ? (const uint32_t *)(d + o_u) : nullptr,
                           (const uint32_t *)nullptr, reinterpret_cast<bigsi_score::HitScore *>(d + o_out));
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpy(scores, d + o_out, n * sizeof(bigsi_hip_hit_score), hipMemcpyDeviceToHost);
    hipError_t e2 = hipFree(d); (void)e2;
    if (e != hipSuccess) return fail(BIGSI_ERR_HIP, "bigsi_hip_score_presence: %s", hipGetErrorString(e));
    return BIGSI_OK;
}

// k_rank_select on the caller's arrays (include/bigsi_hip_testing.h): no index and no batch -- one upload, the launch rank_select()
// makes (launch_rank_select), one download of the whole output.
extern "C" int bigsi_hip_rank_select_arrays(int device, const uint64_t *hits, uint64_t stride_words, uint32_t wv, uint32_t n_seqs,
                                            const void *counters, uint32_t counter_bytes, const uint32_t *num_unique, const uint32_t *min_kmers,
                                            const uint64_t *excluded, uint32_t limit, uint32_t in_place, uint64_t *out)
{
    if (!hits || !out) return fail(BIGSI_ERR_INVALID, "NULL argument");
    if (limit == 0) return fail(BIGSI_ERR_INVALID, "limit is 0");
    if (wv > stride_words) return fail(BIGSI_ERR_INVALID, "wv %u exceeds the stride of %llu words", wv, (unsigned long long)stride_words);
    if (counters && counter_bytes != 2 && counter_bytes != 4) return fail(BIGSI_ERR_INVALID, "counter_bytes %u is neither 2 nor 4", counter_bytes);
    if (counters && (!num_unique || !min_kmers)) return fail(BIGSI_ERR_INVALID, "counters without num_unique and min_kmers");
    if (n_seqs > 0x7FFFFFFFu || stride_words > (1ull << 26)) return fail(BIGSI_ERR_INVALID, "too large for one call");
    if (n_seqs == 0) return BIGSI_OK;
    HIP_TRY(hipSetDevice(device));
    const size_t words = (size_t)n_seqs * stride_words, n_count = counters ? words * 64 * counter_bytes : 0;
    const size_t o_out = round_up(words * 8, 256), o_cnt = round_up(o_out + words * 8, 256), o_nu = round_up(o_cnt + n_count, 256);
    const size_t o_mk = round_up(o_nu + n_seqs * 4ull, 256), o_ex = round_up(o_mk + n_seqs * 4ull, 256), total = o_ex + (size_t)wv * 8 + 8;
    uint8_t *d = nullptr;
    HIP_TRY(hipMalloc((void **)&d, total));
    uint64_t *d_hits = reinterpret_cast<uint64_t *>(d), *d_out = in_place ? d_hits : reinterpret_cast<uint64_t *>(d + o_out);
    hipError_t e = hipMemcpy(d_hits, hits, words * 8, hipMemcpyHostToDevice);
    if (e == hipSuccess && !in_place) e = hipMemcpy(d_out, out, words * 8, hipMemcpyHostToDevice);      // (the caller's preset)
    if (e == hipSuccess && counters) e = hipMemcpy(d + o_cnt, counters, n_count, hipMemcpyHostToDevice);
    if (e == hipSuccess && counters) e = hipMemcpy(d + o_nu, num_unique, n_seqs * 4ull, hipMemcpyHostToDevice);
    if (e == hipSuccess && counters) e = hipMemcpy(d + o_mk, min_kmers, n_seqs * 4ull, hipMemcpyHostToDevice);
    if (e == hipSuccess && excluded && wv) e = hipMemcpy(d + o_ex, excluded, (size_t)wv * 8, hipMemcpyHostToDevice);
    if (e == hipSuccess) {
        launch_rank_select(n_seqs, d_hits, stride_words, wv, counters ? d + o_cnt : nullptr, counter_bytes, (const uint32_t *)(d + o_nu),
                           (const uint32_t *)(d + o_mk), excluded ? (const uint64_t *)(d + o_ex) : nullptr, limit, d_out, 0);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e == hipSuccess) e = hipMemcpy(out, d_out, words * 8, hipMemcpyDeviceToHost);
    hipError_t e2 = hipFree(d); (void)e2;
    if (e != hipSuccess) return fail(BIGSI_ERR_HIP, "bigsi_hip_rank_select_arrays: %s", hipGetErrorString(e));
    return BIGSI_OK;
}

// ------------------------------------------------------------------------------ one-call / streaming searches: stage, export, collect
int bigsi_batch_stage(bigsi_hip_index *ix, bigsi_hip_batch **pb, const char *seqs, const uint64_t *offsets, uint32_t n_seqs, uint32_t k)
{
    TRY(check_batch_args(ix, seqs, offsets, n_seqs, k));
    TRY(use_device(ix));
    bigsi_hip_batch *b = *pb;
    if (!b) {
        b = new (std::nothrow) bigsi_hip_batch();
        if (!b) return fail(BIGSI_ERR_NOMEM, "host allocation failed");
        b->ix = ix;
        *pb = b;
    } else {
        if (b->elements) return fail(BIGSI_ERR_STATE, "a batch of explicit k-mers cannot be reloaded: create a new one");
        TRY(batch_quiesce(b));                                         // this batch's earlier run ...
        if (b->exp_serial) TRY(export_wait(b));                        // ... and the export of its results
    }
    return batch_load(b, seqs, offsets, n_seqs, k, true);
}

// the pinned block an export writes, the flag its last workgroup raises, and the export's serial number
static int export_prepare(bigsi_hip_batch *b, hipStream_t st)
{
    HitBufs &hb = b->hits;
    const uint32_t n = b->n_seqs;
    // (room in the pinned block for the hit lists the export carries along: 16 per sequence -- a read stream whose reads match a
    // handful of samples each then never takes the slower fetch route; the block is only written as far as there are hits)
    const uint64_t spec = export_spec(n, hb.capacity());
    const size_t o_uniq = (n + 2ull) * 8, o_col = o_uniq + ((3ull * n + 1) & ~1ull) * 4, bytes = o_col + 8 * spec;
    TRY(pinned_reserve(&b->pin_out, &b->pin_out_cap, bytes));
    // completion: the kernel's last workgroup writes the export's serial into a pinned word the host spins on (no event record, no
    // hipEventSynchronize: a 1 kbp query's call is ~57 us, of which an event wait is several)
    if (!b->pin_flag) {
        HIP_TRY(hipHostMalloc((void **)&b->pin_flag, 64, hipHostMallocCoherent | hipHostMallocMapped));
        *b->pin_flag = 0;
        TRY(b->exp_count.reserve(256));
        HIP_TRY(hipMemsetAsync(b->exp_count.p, 0, 256, st));
    }
    b->exp_spec = (uint32_t)spec;
    b->path.exp_spec = (uint32_t)spec;
    b->exp_serial++;
    b->exp_stream = st;
    return BIGSI_OK;
}

int bigsi_batch_export(bigsi_hip_batch *b)
{
    if (!b || !b->ran) return fail(BIGSI_ERR_STATE, "bigsi_hip_batch_run has not completed for this batch");
    if (!b->compacted) return fail(BIGSI_ERR_STATE, "internal: export of a run without hit lists");
    if (b->exported_inline) return BIGSI_OK;          // (one read: its kernel wrote the block and raises the flag)
    HitBufs &hb = b->hits;
    hipStream_t st = b->run_stream ? b->run_stream : b->ix->stream;
    const uint32_t n = b->n_seqs;
    TRY(export_prepare(b, st));
    const uint64_t spec = b->exp_spec;
    if (b->fused_run) {
        // a read run: its export also puts the hit lists in query order (k_export_reads); workgroups own ranges of queries
        // (queries per workgroup, A/B at 1000 reads in one call: 1024 -> 51.2 us, 256 -> 47.7, 64 -> 47.8)
        const unsigned rgrid = (unsigned)std::min<uint64_t>(ceil_div(n, (uint64_t)kBlock), 64);
        hipLaunchKernelGGL(k_export_reads, dim3(std::max(rgrid, 1u)), dim3(kBlock), 0, st, hb.q_start.as<uint64_t>(), hb.q_cnt.as<uint32_t>(), n,
                           b->uniq.as<uint32_t>(), hb.col(), hb.cnt(), hb.capacity(), (uint32_t)spec, static_cast<uint64_t *>(b->pin_out), b->exp_count.as<uint32_t>(),
                           (volatile uint64_t *)b->pin_flag, b->exp_serial);
        HIP_TRY(hipGetLastError());
        return BIGSI_OK;
    }
    // the hits it carries along speculatively are few: one workgroup unless the batch is large (one workgroup needs no counter)
    const unsigned grid = (unsigned)std::min<uint64_t>(ceil_div(std::max<uint64_t>(3ull * n, spec), 4 * kBlock), 64);
    hipLaunchKernelGGL(k_export_results, dim3(std::max(grid, 1u)), dim3(kBlock), 0, st, hb.hit_off.as<uint64_t>(), n, b->fused_run ? 1u : 0u, b->uniq.as<uint32_t>(),
                       hb.col(), hb.cnt(), (uint32_t)spec, static_cast<uint64_t *>(b->pin_out), b->exp_count.as<uint32_t>(),
                       (volatile uint64_t *)b->pin_flag, b->exp_serial);
    HIP_TRY(hipGetLastError());
    return BIGSI_OK;
}

// host-side wait for the last export of the batch: spin on the pinned flag for a while (a latency-bound call is over in tens of
// microseconds), then block on the stream (a throughput batch takes milliseconds: no point burning a core)
static int export_wait(bigsi_hip_batch *b)
{
    if (!b->exp_serial) return fail(BIGSI_ERR_STATE, "internal: nothing exported");
    volatile uint64_t *f = b->pin_flag;
    const uint64_t want = b->exp_serial;
    for (uint32_t spins = 0; *f != want; spins++) {
        __builtin_ia32_pause();
        if (spins >= 20000) {                    // ~0.5 ms
            HIP_TRY(hipStreamSynchronize(b->exp_stream));
            if (*f != want) return fail(BIGSI_ERR_HIP, "internal: export finished without raising its flag");
            break;
        }
    }
    __atomic_thread_fence(__ATOMIC_ACQUIRE);
    return BIGSI_OK;
}

// outputs as bigsi_hip_batch_fetch_unique + fetch_hits (hit_offsets relative to this batch, n_seqs + 1 entries)
int bigsi_batch_collect(bigsi_hip_batch *b, uint32_t *num_kmers, uint32_t *num_unique, uint32_t *min_kmers, uint64_t *hit_offsets,
                        uint32_t *colours, uint32_t *counts, uint64_t capacity)
{
    if (!b) return fail(BIGSI_ERR_STATE, "internal: nothing exported");
    TRY(use_device(b->ix));
    TRY(export_wait(b));
    HitBufs &hb = b->hits;
    const uint32_t n = b->n_seqs;
    const uint64_t *off = static_cast<const uint64_t *>(b->pin_out);
    const uint64_t total = off[n];
    if (total > hb.capacity() || (b->fused_run && total > b->exp_spec)) {
        // rare: hit lists that outgrew the device buffers (the general route regrows them and repeats the launch), or a read
        // run with more hits than its export carried along (their query order is made on the host)
        b->path.collect_fetch = 1;
        TRY(bigsi_hip_batch_fetch_unique(b, num_kmers, num_unique, min_kmers));
        const int rc2 = bigsi_hip_batch_fetch_hits(b, hit_offsets, colours, counts, capacity);
        b->idle = !b->job.pending;
        return rc2;
    }
    b->idle = !b->job.pending;          // the export ran behind everything the run queued on its stream
    const uint32_t *u32 = reinterpret_cast<const uint32_t *>(off + n + 2);
    b->h_uniq.assign(u32, u32 + 3ull * n);
    b->h_num_kmers.assign(u32, u32 + n);
    b->h_num_unique.assign(u32 + n, u32 + 2ull * n);
    b->h_min_kmers.assign(u32 + 2ull * n, u32 + 3ull * n);
    b->host_counts_valid = true;
    if (num_kmers) memcpy(num_kmers, u32, n * 4ull);
    if (num_unique) memcpy(num_unique, u32 + n, n * 4ull);
    if (min_kmers) memcpy(min_kmers, u32 + 2ull * n, n * 4ull);
    if (hit_offsets) memcpy(hit_offsets, off, (n + 1ull) * 8);
    if (total > capacity)
        return fail(BIGSI_ERR_CAPACITY, "hit buffers hold %llu entries, %llu needed", (unsigned long long)capacity, (unsigned long long)total);
    const uint32_t *pcol = u32 + ((3ull * n + 1) & ~1ull), *pcnt = pcol + b->exp_spec;
    const uint64_t m = std::min<uint64_t>(total, b->exp_spec);
    if (m && colours) memcpy(colours, pcol, m * 4);
    if (m && counts) memcpy(counts, pcnt, m * 4);
    if (total > m) {          // more hits than the export carried along: the rest by plain copies
        if (colours) HIP_TRY(hipMemcpy(colours + m, hb.col() + m, (total - m) * 4, hipMemcpyDeviceToHost));
        if (counts) HIP_TRY(hipMemcpy(counts + m, hb.cnt() + m, (total - m) * 4, hipMemcpyDeviceToHost));
    }
    return BIGSI_OK;
}

// one-shot KmerSignatureIndex.lookup for an explicit k-mer list: every k-mer is its own one-window sequence, so K1's
// row ids land contiguously (u x h) and one k_lookup launch covers them all.
extern "C" int bigsi_hip_lookup(bigsi_hip_index *ix, const char *kmers, uint32_t k, uint64_t u, uint8_t *out_rows)
{
    BIGSI_ENTER(ix);
    if (!ix || (u && (!kmers || !out_rows))) return fail(BIGSI_ERR_INVALID, "NULL argument");
    if (k == 0) return fail(BIGSI_ERR_INVALID, "k must be > 0");
    if (u == 0) return BIGSI_OK;
    if (u > 0x7FFFFFFFull) return fail(BIGSI_ERR_INVALID, "too many k-mers for one call");
    if (ix->n_cols == 0) return fail(BIGSI_ERR_STATE, "index has no columns");
    std::vector<uint64_t> off(u + 1);
    for (uint64_t i = 0; i <= u; i++) off[i] = i * k;
    bigsi_hip_batch *b = nullptr;
    TRY(bigsi_hip_batch_create(ix, kmers, off.data(), (uint32_t)u, k, &b));
    int rc = run_kmerize(b, 1.0, k1_plan(b, false));
    const uint64_t wv = ix->wv(), rb = ix->rb();
    if (rc == BIGSI_OK) rc = b->scratch.reserve((size_t)u * wv * 8);
    if (rc == BIGSI_OK) {
        const uint64_t wblocks = ceil_div(wv, kBlock);
        if (wblocks * u > 0x7FFFFFFFull) rc = fail(BIGSI_ERR_INVALID, "lookup too large for one launch");
        else {
            hipLaunchKernelGGL(k_lookup, dim3((unsigned)(wblocks * u)), dim3(kBlock), 0, ix->stream, ix->d_index, ix->stride_words, (uint32_t)wv,
                               b->rows.as<uint64_t>(), ix->h, (uint32_t)u, b->scratch.as<uint64_t>());
            hipError_t e = hipGetLastError();
            if (e == hipSuccess) e = hipMemcpy2DAsync(out_rows, rb, b->scratch.p, wv * 8, rb, u, hipMemcpyDeviceToHost, ix->stream);
            if (e == hipSuccess) e = hipStreamSynchronize(ix->stream);
            if (e != hipSuccess) rc = fail(BIGSI_ERR_HIP, "bigsi_hip_lookup: %s", hipGetErrorString(e));
        }
    }
    bigsi_hip_batch_destroy(b);
    return rc;
}

// KmerSignatureIndex.lookup for explicit, already canonical elements of any byte lengths (non-ASCII k-mers): every element is
// its own one-position sequence of an element batch, k_rows_raw hashes them, one k_lookup launch ANDs their rows.
extern "C" int bigsi_hip_lookup_raw(bigsi_hip_index *ix, const char *blob, const uint64_t *elem_offsets, uint64_t u, uint8_t *out_rows)
{
    BIGSI_ENTER(ix);
    if (!ix || (u && (!elem_offsets || !out_rows))) return fail(BIGSI_ERR_INVALID, "NULL argument");
    if (u == 0) return BIGSI_OK;
    if (u > 0x7FFFFFFFull) return fail(BIGSI_ERR_INVALID, "too many k-mers for one call");
    if (ix->n_cols == 0) return fail(BIGSI_ERR_STATE, "index has no columns");
    std::vector<uint64_t> one(u + 1);
    std::vector<uint32_t> zero(u, 0u);
    for (uint64_t i = 0; i <= u; i++) one[i] = i;
    bigsi_hip_batch *b = nullptr;
    TRY(bigsi_hip_batch_create_elements(ix, blob, elem_offsets, one.data(), zero.data(), one.data(), (uint32_t)u, &b));
    int rc = run_kmerize(b, 1.0, k1_plan(b, false));
    const uint64_t wv = ix->wv(), rb = ix->rb();
    if (rc == BIGSI_OK) rc = b->scratch.reserve((size_t)u * wv * 8);
    if (rc == BIGSI_OK) {
        const uint64_t wblocks = ceil_div(wv, kBlock);
        if (wblocks * u > 0x7FFFFFFFull) rc = fail(BIGSI_ERR_INVALID, "lookup too large for one launch");
        else {
            hipLaunchKernelGGL(k_lookup, dim3((unsigned)(wblocks * u)), dim3(kBlock), 0, ix->stream, ix->d_index, ix->stride_words, (uint32_t)wv,
                               b->rows.as<uint64_t>(), ix->h, (uint32_t)u, b->scratch.as<uint64_t>());
            hipError_t e = hipGetLastError();
            if (e == hipSuccess) e = hipMemcpy2DAsync(out_rows, rb, b->scratch.p, wv * 8, rb, u, hipMemcpyDeviceToHost, ix->stream);
            if (e == hipSuccess) e = hipStreamSynchronize(ix->stream);
            if (e != hipSuccess) rc = fail(BIGSI_ERR_HIP, "bigsi_hip_lookup_raw: %s", hipGetErrorString(e));
        }
    }
    bigsi_hip_batch_destroy(b);
    return rc;
}
