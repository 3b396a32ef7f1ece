// bigsi_cpu.cpp -- libbigsi_cpu.so: the CPU twin of the CORE layer of libbigsi_hip.so (include/bigsi_cpu.h).
//
// The BIGSI query path computed on the host in the reference's own shape, behind the same C boundary: a host without a GPU binds
// it explicitly, bench.py times it as the CPU baseline THROUGH the product boundary, and tests/c_host/search_host.c builds
// against either library.  The hip-hbm backend never loads this file: there is no CPU fallback.
//
// Default search path = what the reference does per query (file:line relative to the reference root):
//   seq_to_kmers                  utils/fncts.py:63-65     every k-window of the raw bytes
//   set(kmers)                    graph/index.py:45        unique query k-mers (first-occurrence order kept for presence)
//   canonical                     utils/fncts.py:38-54     reverse complement as a new string, lexicographic min
//   generate_hashes               bloom/bloomfilter.py:5-13 mmh3 (MurmurHash3_x86_32, signed) % m with Python's floor-mod, h seeds
//   batch_get + frombytes         storage/base.py:58-59,96-109  the union of rows fetched ONCE, each COPIED out of the store
//   bitwise_and                   utils/fncts.py:24-25     a fresh buffer per AND step
//   exact_filter                  graph/bigsi.py:192-205   AND of all k-mer rows, set bits ascending
//   unpack_and_sum + threshold    graph/bigsi.py:35-44,211-230,241-242  one int32 per bit, added; count >= ceil(u * threshold)
// BIGSI_CPU_WORD_PARALLEL replaces the last four by 64-bit word operations on the resident rows (same results).
// Row format = the reference's bitarray.tobytes(): column c at byte c / 8 under mask 0x80 >> (c % 8).
#include "bigsi_cpu.h"
#include "bigsi_cpu_collapse.h"
#include "bigsi_cpu_compact.h"
#include "bigsi_cpu_consensus.h"
#include "bigsi_cpu_fold.h"
#include "bigsi_cpu_kmercount.h"
#include "bigsi_cpu_pairwise.h"
#include "bigsi_cpu_prevalence.h"
#include "bigsi_cpu_window.h"
#include "bigsi_cpu_tally.h"
#include "bigsi_cpu_classify.h"
#include "bigsi_cpu_associate.h"
#include "bigsi_cpu_genotype.h"
#include "bigsi_cpu_typing.h"

#include <math.h>
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <atomic>
#include <map>
#include <new>
#include <string>
#include <string_view>
#include <unordered_map>
#include <vector>

#include <fcntl.h>
#include <mutex>

#include "../csrc/bigsi_bdb.hpp"
#include "../csrc/bigsi_score.hpp"

namespace {

thread_local char g_err[512] = "";

int fail(int code, const char *fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof g_err, fmt, ap);
    va_end(ap);
    return code;
}

#define TRY(expr)            \
    do {                     \
        int rc_ = (expr);    \
        if (rc_ != BIGSI_OK) \
            return rc_;      \
    } while (0)

inline uint64_t ceil_div(uint64_t a, uint64_t b) { return (a + b - 1) / b; }
inline uint64_t round_up(uint64_t a, uint64_t b) { return ceil_div(a, b) * b; }

// ---------------------------------------------------------------------------------------------- hashing
inline uint32_t rotl(uint32_t x, int r) { return (x << r) | (x >> (32 - r)); }

// MurmurHash3_x86_32 (Austin Appleby, public domain): what mmh3.hash(str, seed) computes over the UTF-8 bytes
uint32_t murmur3(const uint8_t *p, size_t len, uint32_t seed)
{
    uint32_t h = seed;
    const size_t nb = len / 4;
    for (size_t i = 0; i < nb; i++) {
        uint32_t k;
        memcpy(&k, p + 4 * i, 4);             // little-endian host
        k *= 0xcc9e2d51u; k = rotl(k, 15); k *= 0x1b873593u;
        h ^= k; h = rotl(h, 13); h = h * 5u + 0xe6546b64u;
    }
    uint32_t k = 0;
    const uint8_t *t = p + 4 * nb;
    const size_t rem = len & 3;
    if (rem == 3) k ^= (uint32_t)t[2] << 16;
    if (rem >= 2) k ^= (uint32_t)t[1] << 8;
    if (rem >= 1) { k ^= t[0]; k *= 0xcc9e2d51u; k = rotl(k, 15); k *= 0x1b873593u; h ^= k; }
    h ^= (uint32_t)len;
    h ^= h >> 16; h *= 0x85ebca6bu; h ^= h >> 13; h *= 0xc2b2ae35u; h ^= h >> 16;
    return h;
}

// Python: mmh3.hash(...) % m  (signed hash, result in [0, m))
uint64_t floor_mod_row(uint32_t hash, uint64_t m)
{
    const int64_t s = (int32_t)hash;
    const int64_t r = s % (int64_t)m;       // C: sign of the dividend
    return (uint64_t)(r < 0 ? r + (int64_t)m : r);
}

inline char comp(char c)
{
    switch (c) {
    case 'A': return 'T';
    case 'T': return 'A';
    case 'C': return 'G';
    case 'G': return 'C';
    default: return c;              // COMPLEMENT.get(base, base): lowercase, N, anything else unchanged
    }
}

// canonical(k-mer) into `out` (a std::string reused by the caller)
void canonical(const char *s, uint32_t k, std::string &out)
{
    out.resize(k);
    for (uint32_t i = 0; i < k; i++) out[i] = comp(s[k - 1 - i]);
    if (memcmp(s, out.data(), k) <= 0) out.assign(s, k);          // sorted([kmer, rc])[0]
}

// ---------------------------------------------------------------------------------------------- synthetic contents
// the generator of bigsi_hip_fill_synthetic (csrc/bigsi_kernels.hpp: k_fill_synth), restated: word w of row r is the AND of
// `draws` values of a counter-based hash of (seed, shard, r, w), pad bits cleared
inline uint64_t mix64(uint64_t x)
{
    x += 0x9E3779B97F4A7C15ull;
    x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
    x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
    return x ^ (x >> 31);
}

uint64_t valid_word_mask(uint64_t w, uint64_t n_cols)
{
    const uint64_t c0 = w * 64;
    if (c0 + 64 <= n_cols) return ~0ull;
    if (c0 >= n_cols) return 0;
    uint64_t mask = 0;
    for (int b = 0; b < 8; b++) {
        const uint64_t cb = c0 + 8ull * b, left = cb >= n_cols ? 0 : std::min<uint64_t>(n_cols - cb, 8);
        mask |= (uint64_t)((0xFFu << (8 - left)) & 0xFFu) << (8 * b);
    }
    return mask;
}

}  // namespace

// rows served from a BerkeleyDB hash FILE (bigsi_cpu_open_bdb) instead of a table in RAM: where every "<row>:bitarray" record lies
struct BdbRows {
    int fd = -1;
    BigsiBdb db;
    std::vector<BigsiBdb::Loc> loc;
    // errno of the first record read that failed since the last check (an I/O error, a corrupt overflow chain): the entry point that
    // was reading fails with it instead of answering from a zero / partial row (bdb_read_failed below; fork-pool workers have their own copy)
    mutable std::atomic<int> io_error{0};
    void note(int e) const { int none = 0; if (e) io_error.compare_exchange_strong(none, e); }
};

struct bigsi_cpu_index {
    uint64_t m = 0, n_cols = 0, cap_cols = 0, stride = 0;      // stride: bytes per row, a multiple of 128 like the device's pitch
    uint64_t alloc_rows = 0;      // rows the table behind `rows` holds: m, or more between bigsi_cpu_fold_rows and bigsi_cpu_trim_rows
    uint32_t h = 0;
    uint8_t *rows = nullptr;
    BdbRows *bdb = nullptr;      // non-null: no table in RAM, every row fetch reads the store's file (read-only index)
    // row r's first rb bytes: the table's own memory, or -- BerkeleyDB store -- read into `tmp` (zero-extended), as a KV store's get does
    const uint8_t *fetch(uint64_t r, uint64_t rb_, std::vector<uint8_t> &tmp, std::vector<uint8_t> &page) const
    {
        if (!bdb) return rows + r * stride;
        tmp.assign(rb_, 0);
        const BigsiBdb::Loc &l = bdb->loc[r];
        if (l.kind) bdb->note(bdb->db.read_value(l, tmp.data(), (uint32_t)std::min<uint64_t>(l.len, rb_), page));
        return tmp.data();
    }
    uint64_t rb() const { return ceil_div(n_cols, 8); }
    uint8_t *row(uint64_t r) { return rows + r * stride; }
    const uint8_t *row(uint64_t r) const { return rows + r * stride; }
};

namespace {

uint64_t stride_for(uint64_t cols) { return std::max<uint64_t>(128, round_up(ceil_div(cols, 64) * 8, 128)); }

// the result of an entry point that read rows: BIGSI_OK, or -- a BerkeleyDB-backed index whose file could not be read -- the failure
int bdb_read_failed(const bigsi_cpu_index *ix)
{
    if (!ix->bdb) return BIGSI_OK;
    const int e = ix->bdb->io_error.exchange(0);
    return e ? fail(BIGSI_ERR_INVALID, "reading a record of the BerkeleyDB store failed: %s%s%s", strerror(e), ix->bdb->db.error.empty() ? "" : ": ",
                    ix->bdb->db.error.c_str())
             : BIGSI_OK;
}

// BIGSI_OK, or the refusal of every call that would write to a BerkeleyDB-backed index or sweep all of its rows (NULL passes: the
// caller's own check names it)
int read_only(const bigsi_cpu_index *ix)
{
    if (ix && ix->bdb)
        return fail(BIGSI_ERR_STATE, "this index serves its rows from a BerkeleyDB file (bigsi_cpu_open_bdb): read-only, search / lookup / get_rows / presence only");
    return BIGSI_OK;
}

// The calls that make one index from another (extract_columns, collapse_columns_into, fold_rows_into): what the two must have in
// common, in the order of the device library's check_derive (no devices, handles or views here).  An entry point checks its own
// arguments before this.
struct DeriveRule {
    const char *in_place;      // the in-place form a caller may have meant, or nullptr: there is none
    bool rows_divide;          // the destination's num_rows divides the source's (a fold); otherwise the two are equal
    bool same_hashes;
};

int check_derive(const DeriveRule &r, const bigsi_cpu_index *dst, const bigsi_cpu_index *src)
{
    TRY(read_only(dst));
    if (!dst || !src) return fail(BIGSI_ERR_INVALID, "NULL argument");
    if (dst == src)
        return fail(BIGSI_ERR_INVALID, "dst and src are the same index (%s%s)", r.in_place ? r.in_place : "there is no in-place form", r.in_place ? " works in place" : "");
    if (r.rows_divide ? (dst->m == 0 || src->m % dst->m) : dst->m != src->m)
        return fail(BIGSI_ERR_INVALID, r.rows_divide ? "the destination's num_rows %llu does not divide the source's %llu" : "row counts differ (%llu vs %llu)",
                    (unsigned long long)dst->m, (unsigned long long)src->m);
    if (r.same_hashes && dst->h != src->h) return fail(BIGSI_ERR_INVALID, "num_hashes differ (%u vs %u)", dst->h, src->h);
    if (dst->n_cols != 0) return fail(BIGSI_ERR_STATE, "the destination already holds %llu column(s)", (unsigned long long)dst->n_cols);
    return BIGSI_OK;
}

int check_seqs(const char *seqs, const uint64_t *offsets, uint64_t n_seqs, uint32_t k)
{
    if (!offsets) return fail(BIGSI_ERR_INVALID, "NULL argument");
    if (n_seqs == 0) return fail(BIGSI_ERR_INVALID, "a batch needs at least one sequence");
    if (k == 0) return fail(BIGSI_ERR_INVALID, "k must be > 0");
    for (uint64_t i = 0; i < n_seqs; i++)
        if (offsets[i + 1] < offsets[i]) return fail(BIGSI_ERR_INVALID, "offsets must be non-decreasing");
    if (offsets[n_seqs] - offsets[0] && !seqs) return fail(BIGSI_ERR_INVALID, "seqs is NULL");
    return BIGSI_OK;
}

// the h rows of one (canonical) element, seeds 0 .. h-1
inline void rows_of(const std::string &canon, uint32_t h, uint64_t m, uint64_t *out)
{
    for (uint32_t s = 0; s < h; s++) out[s] = floor_mod_row(murmur3(reinterpret_cast<const uint8_t *>(canon.data()), canon.size(), s), m);
}

struct QueryKmers {
    std::vector<uint32_t> first_pos;       // unique k-mers in first-occurrence order: position of the first occurrence
    std::vector<uint32_t> pos_unique;      // every position -> index of its unique k-mer
};

void unique_kmers(const char *s, uint64_t len, uint32_t k, QueryKmers &q)
{
    q.first_pos.clear();
    q.pos_unique.clear();
    if (len < k) return;
    const uint64_t n = len - k + 1;
    std::unordered_map<std::string_view, uint32_t> seen;
    seen.reserve(n * 2);
    q.pos_unique.resize(n);
    for (uint64_t i = 0; i < n; i++) {
        auto it = seen.emplace(std::string_view(s + i, k), (uint32_t)q.first_pos.size());
        if (it.second) q.first_pos.push_back((uint32_t)i);
        q.pos_unique[i] = it.first->second;
    }
}

struct Hits {
    uint64_t *off;
    uint32_t *col, *cnt;
    uint64_t cap, total = 0;
    void push(uint32_t c, uint32_t n)
    {
        if (total < cap) {
            if (col) col[total] = c;
            if (cnt) cnt[total] = n;
        }
        total++;
    }
};

// one sequence, the reference's shape
void search_reference_shaped(const bigsi_cpu_index *ix, const char *s, uint64_t len, uint32_t k, double threshold, QueryKmers &q,
                             uint32_t *nk, uint32_t *nu, uint32_t *mk, Hits &hits)
{
    unique_kmers(s, len, k, q);
    const uint32_t u = (uint32_t)q.first_pos.size(), h = ix->h;
    const uint64_t rb = ix->rb(), n_cols = ix->n_cols;
    *nk = (uint32_t)q.pos_unique.size();
    *nu = u;
    const uint32_t min_kmers = (uint32_t)ceil((double)u * threshold);        // math.ceil(len(set(kmers)) * threshold), graph/bigsi.py:179
    *mk = min_kmers;
    const bool exact = threshold == 1.0;
    if (u == 0) {
        if (!exact)                                 // counts are all zero and min_kmers is 0: every sample passes `count >= 0`
            for (uint64_t c = 0; c < n_cols; c++) hits.push((uint32_t)c, 0);
        return;
    }
    // {k-mer -> set(rows)}, the union of rows fetched once and copied out of the store (batch_get + frombytes)
    std::vector<uint64_t> kmer_rows((size_t)u * h);
    std::unordered_map<uint64_t, uint32_t> fetched;
    std::vector<std::vector<uint8_t>> row_copy;
    std::vector<uint8_t> bdb_page;
    std::string canon;
    for (uint32_t j = 0; j < u; j++) {
        canonical(s + q.first_pos[j], k, canon);
        rows_of(canon, h, ix->m, &kmer_rows[(size_t)j * h]);
        for (uint32_t t = 0; t < h; t++) {
            const uint64_t r = kmer_rows[(size_t)j * h + t];
            if (fetched.emplace(r, (uint32_t)row_copy.size()).second) {
                if (ix->bdb) {          // the store's get(): the record's bytes read from the file (an overflow chain of pages for wide rows)
                    row_copy.emplace_back(rb, 0);
                    const BigsiBdb::Loc &l = ix->bdb->loc[r];
                    if (l.kind) ix->bdb->note(ix->bdb->db.read_value(l, row_copy.back().data(), (uint32_t)std::min<uint64_t>(l.len, rb), bdb_page));
                } else row_copy.emplace_back(ix->row(r), ix->row(r) + rb);
            }
        }
    }
    std::vector<uint8_t> all;                        // exact: AND of every k-mer's row
    std::vector<int32_t> sums;                       // inexact: one int32 per bit
    if (!exact) sums.assign(rb * 8, 0);
    for (uint32_t j = 0; j < u; j++) {
        std::vector<uint8_t> acc(row_copy[fetched[kmer_rows[(size_t)j * h]]]);               // reduce(x & y): a new bitarray per step
        for (uint32_t t = 1; t < h; t++) {
            const std::vector<uint8_t> &other = row_copy[fetched[kmer_rows[(size_t)j * h + t]]];
            std::vector<uint8_t> next(rb);
            for (uint64_t b = 0; b < rb; b++) next[b] = acc[b] & other[b];
            acc.swap(next);
        }
        if (exact) {
            if (j == 0) all = acc;
            else {
                std::vector<uint8_t> next(rb);
                for (uint64_t b = 0; b < rb; b++) next[b] = all[b] & acc[b];
                all.swap(next);
            }
        } else {
            // unpack(one byte per bit) -> int32 -> add (graph/bigsi.py:35-44)
            std::vector<int32_t> unpacked(rb * 8);
            for (uint64_t b = 0; b < rb; b++)
                for (int bit = 0; bit < 8; bit++) unpacked[b * 8 + bit] = (acc[b] >> (7 - bit)) & 1;
            for (uint64_t c = 0; c < rb * 8; c++) sums[c] += unpacked[c];
        }
    }
    if (exact) {
        for (uint64_t c = 0; c < n_cols; c++)
            if (all[c >> 3] & (0x80u >> (c & 7))) hits.push((uint32_t)c, u);
    } else {
        for (uint64_t c = 0; c < n_cols; c++)
            if ((uint32_t)sums[c] >= min_kmers) hits.push((uint32_t)c, (uint32_t)sums[c]);
    }
}

// the same results on 64-bit words of the resident rows: no copies, counters touched only where bits are set
void search_word_parallel(const bigsi_cpu_index *ix, const char *s, uint64_t len, uint32_t k, double threshold, QueryKmers &q,
                          uint32_t *nk, uint32_t *nu, uint32_t *mk, Hits &hits)
{
    unique_kmers(s, len, k, q);
    const uint32_t u = (uint32_t)q.first_pos.size(), h = ix->h;
    const uint64_t n_cols = ix->n_cols, words = ceil_div(n_cols, 64);
    *nk = (uint32_t)q.pos_unique.size();
    *nu = u;
    const uint32_t min_kmers = (uint32_t)ceil((double)u * threshold);
    *mk = min_kmers;
    const bool exact = threshold == 1.0;
    if (u == 0) {
        if (!exact)
            for (uint64_t c = 0; c < n_cols; c++) hits.push((uint32_t)c, 0);
        return;
    }
    std::vector<uint64_t> kr((size_t)u * h);
    std::string canon;
    for (uint32_t j = 0; j < u; j++) {
        canonical(s + q.first_pos[j], k, canon);
        rows_of(canon, h, ix->m, &kr[(size_t)j * h]);
    }
    auto word = [&](uint64_t r, uint64_t w) { uint64_t v; memcpy(&v, ix->row(r) + 8 * w, 8); return v; };
    auto col_of_bit = [](uint64_t w, int bit) { return w * 64 + (uint64_t)(bit >> 3) * 8 + 7 - (bit & 7); };      // little-endian load of row bytes
    std::vector<uint32_t> sums;
    if (!exact) sums.assign(words * 64, 0);
    std::vector<uint64_t> all(exact ? words : 0, ~0ull);
    for (uint32_t j = 0; j < u; j++)
        for (uint64_t w = 0; w < words; w++) {
            uint64_t a = word(kr[(size_t)j * h], w);
            for (uint32_t t = 1; t < h; t++) a &= word(kr[(size_t)j * h + t], w);
            if (exact) all[w] &= a;
            else
                while (a) {
                    const int bit = __builtin_ctzll(a);
                    a &= a - 1;
                    sums[col_of_bit(w, bit)]++;
                }
        }
    if (exact) {
        for (uint64_t c = 0; c < n_cols; c++) {
            const uint64_t w = c >> 6;
            const int bit = (int)(((c >> 3) & 7) * 8 + 7 - (c & 7));
            if ((all[w] >> bit) & 1) hits.push((uint32_t)c, u);
        }
    } else {
        for (uint64_t c = 0; c < n_cols; c++)
            if (sums[c] >= min_kmers) hits.push((uint32_t)c, sums[c]);
    }
}

}  // namespace

extern "C" {

const char *bigsi_cpu_last_error(void) { return g_err; }

int bigsi_cpu_device_count(int *out)
{
    if (!out) return fail(BIGSI_ERR_INVALID, "NULL argument");
    *out = 1;
    return BIGSI_OK;
}

int bigsi_cpu_open(uint64_t num_rows, uint64_t num_cols, uint64_t col_capacity, uint32_t num_hashes, int, bigsi_cpu_index **out)
{
    if (!out) return fail(BIGSI_ERR_INVALID, "out is NULL");
    *out = nullptr;
    if (num_rows == 0) return fail(BIGSI_ERR_INVALID, "num_rows must be > 0");
    if (num_hashes == 0) return fail(BIGSI_ERR_INVALID, "num_hashes must be > 0");
    col_capacity = std::max<uint64_t>(std::max(col_capacity, num_cols), 1);
    bigsi_cpu_index *ix = new (std::nothrow) bigsi_cpu_index();
    if (!ix) return fail(BIGSI_ERR_NOMEM, "host allocation failed");
    ix->m = num_rows;
    ix->alloc_rows = num_rows;
    ix->n_cols = num_cols;
    ix->h = num_hashes;
    ix->stride = stride_for(col_capacity);
    ix->cap_cols = ix->stride * 8;
    ix->rows = static_cast<uint8_t *>(calloc(ix->m, ix->stride));
    if (!ix->rows) { delete ix; return fail(BIGSI_ERR_NOMEM, "cannot allocate %llu x %llu bytes", (unsigned long long)num_rows, (unsigned long long)ix->stride); }
    *out = ix;
    return BIGSI_OK;
}

int bigsi_cpu_close(bigsi_cpu_index *ix)
{
    if (!ix) return BIGSI_OK;
    free(ix->rows);
    if (ix->bdb) {
        if (ix->bdb->fd >= 0) close(ix->bdb->fd);
        delete ix->bdb;
    }
    delete ix;
    return BIGSI_OK;
}

// An index whose rows stay in the reference's own store: a BerkeleyDB HASH file (bigsi/storage/berkeleydb.py:6-19) holding the
// "<row>:bitarray" records and the index integers of a v0.3 BIGSI index (bigsi/storage/base.py:29-36).  Nothing is loaded: every
// row a search needs is read from the file when it is needed -- located by a table built with one scan of the hash pages (libdb
// finds a record by hashing its key to a bucket page; the table stands in for that), then its bytes gathered from the page, or the
// overflow chain of pages, they lie in.  The closest this package comes to the reference's "berkeleydb / CPU path" without libdb
// (neither bsddb3 nor the db.h headers exist on these hosts): reference-shaped search, lookup, get_rows and presence only.
int bigsi_cpu_open_bdb(const char *path, uint32_t threads, bigsi_cpu_index **out)
{
    if (!path || !out) return fail(BIGSI_ERR_INVALID, "NULL argument");
    *out = nullptr;
    const int fd = open(path, O_RDONLY);
    if (fd < 0) return fail(BIGSI_ERR_INVALID, "%s: %s", path, strerror(errno));
    BdbRows *b = new (std::nothrow) BdbRows();
    bigsi_cpu_index *ix = new (std::nothrow) bigsi_cpu_index();
    if (!b || !ix) { close(fd); delete b; delete ix; return fail(BIGSI_ERR_NOMEM, "host allocation failed"); }
    b->fd = fd;
    ix->bdb = b;
    auto bail = [&](int code, const std::string &msg) { bigsi_cpu_close(ix); return fail(code, "%s: %s", path, msg.c_str()); };
    if (b->db.open_fd(fd)) return bail(BIGSI_ERR_INVALID, b->db.error);
    if (threads == 0) threads = std::min(16u, std::max(1u, std::thread::hardware_concurrency() / 4));
    // the small records first (number_of_rows, number_of_cols, ksi:num_hashes), the row locations in the same pass
    std::mutex mu;
    std::vector<std::pair<uint64_t, BigsiBdb::Loc>> rows;
    std::vector<std::pair<std::string, BigsiBdb::Loc>> small;
    if (b->db.scan(threads, [&](unsigned, const uint8_t *key, uint32_t klen, const BigsiBdb::Loc &l) {
            uint64_t r;
            std::lock_guard<std::mutex> g(mu);
            if (bigsi_bdb_row_key(key, klen, &r)) rows.emplace_back(r, l);
            else if (klen < 64) small.emplace_back(std::string(reinterpret_cast<const char *>(key), klen), l);
        }))
        return bail(BIGSI_ERR_INVALID, b->db.error);
    auto integer = [&](const char *key, uint64_t *v) -> bool {
        std::vector<uint8_t> page;
        for (auto &s_ : small)
            if (s_.first == key && s_.second.len < 32) {
                char buf[32] = {0};
                if (b->db.read_value(s_.second, reinterpret_cast<uint8_t *>(buf), s_.second.len, page)) return false;
                char *end = nullptr;
                *v = strtoull(buf, &end, 10);
                return end != buf;
            }
        return false;
    };
    uint64_t m = 0, n = 0, h = 0;
    if (!integer("number_of_rows:int", &m) || !integer("number_of_cols:int", &n) || !integer("ksi:num_hashes:int", &h) || m == 0 || h == 0)
        return bail(BIGSI_ERR_INVALID, "no number_of_rows / number_of_cols / ksi:num_hashes records: not a BIGSI v0.3 index");
    ix->m = m;
    ix->n_cols = n;
    ix->h = (uint32_t)h;
    ix->stride = stride_for(std::max<uint64_t>(n, 1));
    ix->cap_cols = ix->stride * 8;
    b->loc.assign(m, BigsiBdb::Loc{});
    for (auto &e : rows)
        if (e.first < m) b->loc[e.first] = e.second;
    *out = ix;
    return BIGSI_OK;
}

int bigsi_cpu_get_info(const bigsi_cpu_index *ix, bigsi_hip_info *out)
{
    if (!ix || !out) return fail(BIGSI_ERR_INVALID, "NULL argument");
    out->num_rows = ix->m;
    out->num_cols = ix->n_cols;
    out->col_capacity = ix->cap_cols;
    out->row_bytes = ix->rb();
    out->row_stride_bytes = ix->stride;
    out->index_bytes = ix->m * ix->stride;
    out->num_hashes = ix->h;
    out->device = -1;
    return BIGSI_OK;
}

int bigsi_cpu_set_num_cols(bigsi_cpu_index *ix, uint64_t num_cols)
{
    if (!ix) return fail(BIGSI_ERR_INVALID, "NULL index");
    if (num_cols > ix->cap_cols) return fail(BIGSI_ERR_CAPACITY, "num_cols %llu exceeds col_capacity %llu", (unsigned long long)num_cols, (unsigned long long)ix->cap_cols);
    ix->n_cols = num_cols;
    return BIGSI_OK;
}

int bigsi_cpu_set_num_hashes(bigsi_cpu_index *ix, uint32_t num_hashes)
{
    if (!ix) return fail(BIGSI_ERR_INVALID, "NULL index");
    if (num_hashes == 0) return fail(BIGSI_ERR_INVALID, "num_hashes must be > 0");
    ix->h = num_hashes;
    return BIGSI_OK;
}

int bigsi_cpu_reserve_cols(bigsi_cpu_index *ix, uint64_t col_capacity)
{
    TRY(read_only(ix));
    if (!ix) return fail(BIGSI_ERR_INVALID, "NULL index");
    if (col_capacity <= ix->cap_cols) return BIGSI_OK;
    const uint64_t stride = stride_for(col_capacity);
    uint8_t *grown = static_cast<uint8_t *>(calloc(ix->m, stride));
    if (!grown) return fail(BIGSI_ERR_NOMEM, "cannot allocate %llu x %llu bytes", (unsigned long long)ix->m, (unsigned long long)stride);
    for (uint64_t r = 0; r < ix->m; r++) memcpy(grown + r * stride, ix->row(r), ix->stride);
    free(ix->rows);
    ix->rows = grown;
    ix->alloc_rows = ix->m;
    ix->stride = stride;
    ix->cap_cols = stride * 8;
    return BIGSI_OK;
}

int bigsi_cpu_synchronize(bigsi_cpu_index *ix) { return ix ? BIGSI_OK : fail(BIGSI_ERR_INVALID, "NULL index"); }

int bigsi_cpu_set_rows(bigsi_cpu_index *ix, const uint64_t *row_ids, uint64_t n, const uint8_t *bytes, uint64_t row_bytes)
{
    TRY(read_only(ix));
    if (!ix || (n && (!row_ids || !bytes))) return fail(BIGSI_ERR_INVALID, "NULL argument");
    if (row_bytes > ix->stride) return fail(BIGSI_ERR_CAPACITY, "row_bytes %llu exceeds the row stride %llu", (unsigned long long)row_bytes, (unsigned long long)ix->stride);
    for (uint64_t i = 0; i < n; i++)
        if (row_ids[i] >= ix->m) return fail(BIGSI_ERR_RANGE, "row %llu out of range", (unsigned long long)row_ids[i]);
    for (uint64_t i = 0; i < n; i++) {
        uint8_t *dst = ix->row(row_ids[i]);
        memcpy(dst, bytes + i * row_bytes, row_bytes);
        memset(dst + row_bytes, 0, ix->stride - row_bytes);
    }
    return BIGSI_OK;
}

int bigsi_cpu_get_rows(bigsi_cpu_index *ix, const uint64_t *row_ids, uint64_t n, uint8_t *out, uint64_t row_bytes)
{
    if (!ix || (n && (!row_ids || !out))) return fail(BIGSI_ERR_INVALID, "NULL argument");
    if (row_bytes > ix->stride) return fail(BIGSI_ERR_CAPACITY, "row_bytes %llu exceeds the row stride %llu", (unsigned long long)row_bytes, (unsigned long long)ix->stride);
    for (uint64_t i = 0; i < n; i++)
        if (row_ids[i] >= ix->m) return fail(BIGSI_ERR_RANGE, "row %llu out of range", (unsigned long long)row_ids[i]);
    std::vector<uint8_t> tmp, page;
    for (uint64_t i = 0; i < n; i++) memcpy(out + i * row_bytes, ix->fetch(row_ids[i], row_bytes, tmp, page), row_bytes);
    return bdb_read_failed(ix);
}

int bigsi_cpu_clear(bigsi_cpu_index *ix)
{
    TRY(read_only(ix));
    if (!ix) return fail(BIGSI_ERR_INVALID, "NULL index");
    memset(ix->rows, 0, ix->m * ix->stride);
    return BIGSI_OK;
}

int bigsi_cpu_insert_column(bigsi_cpu_index *ix, uint64_t col, const uint8_t *bloom)
{
    return bigsi_cpu_insert_columns(ix, col, 1, bloom, ix ? ceil_div(ix->m, 8) : 0);
}

int bigsi_cpu_insert_columns(bigsi_cpu_index *ix, uint64_t col0, uint64_t n, const uint8_t *blooms, uint64_t bloom_stride_bytes)
{
    TRY(read_only(ix));
    if (!ix || (n && !blooms)) return fail(BIGSI_ERR_INVALID, "NULL argument");
    if (col0 > ix->n_cols) return fail(BIGSI_ERR_RANGE, "col0 %llu beyond num_cols %llu", (unsigned long long)col0, (unsigned long long)ix->n_cols);
    if (col0 + n > ix->cap_cols) return fail(BIGSI_ERR_CAPACITY, "columns [%llu, %llu) exceed col_capacity %llu", (unsigned long long)col0, (unsigned long long)(col0 + n), (unsigned long long)ix->cap_cols);
    if (n && bloom_stride_bytes < ceil_div(ix->m, 8)) return fail(BIGSI_ERR_INVALID, "bloom_stride_bytes is smaller than a filter");
    for (uint64_t i = 0; i < n; i++) {
        const uint8_t *f = blooms + i * bloom_stride_bytes;
        const uint64_t c = col0 + i;
        const uint8_t mask = (uint8_t)(0x80u >> (c & 7));
        for (uint64_t r = 0; r < ix->m; r++) {
            uint8_t *b = ix->row(r) + (c >> 3);
            if (f[r >> 3] & (0x80u >> (r & 7))) *b |= mask;
            else *b &= (uint8_t)~mask;
        }
    }
    ix->n_cols = std::max(ix->n_cols, col0 + n);
    return BIGSI_OK;
}

int bigsi_cpu_get_column(bigsi_cpu_index *ix, uint64_t col, uint8_t *out)
{
    TRY(read_only(ix));
    if (!ix || !out) return fail(BIGSI_ERR_INVALID, "NULL argument");
    if (col >= ix->n_cols) return fail(BIGSI_ERR_RANGE, "column %llu out of range", (unsigned long long)col);
    memset(out, 0, ceil_div(ix->m, 8));
    for (uint64_t r = 0; r < ix->m; r++)
        if (ix->row(r)[col >> 3] & (0x80u >> (col & 7))) out[r >> 3] |= (uint8_t)(0x80u >> (r & 7));
    return BIGSI_OK;
}

// per column, the rows (of the selected ones) that have its bit: one row at a time, one column at a time
int bigsi_cpu_column_popcounts(bigsi_cpu_index *ix, const uint8_t *row_mask, uint64_t *out, uint64_t capacity)
{
    TRY(read_only(ix));
    if (!ix || !out) return fail(BIGSI_ERR_INVALID, "NULL argument");
    if (capacity < ix->n_cols)
        return fail(BIGSI_ERR_CAPACITY, "capacity %llu is below num_cols %llu", (unsigned long long)capacity, (unsigned long long)ix->n_cols);
    for (uint64_t c = 0; c < ix->n_cols; c++) out[c] = 0;
    for (uint64_t r = 0; r < ix->m; r++) {
        if (row_mask && !(row_mask[r >> 3] & (0x80u >> (r & 7)))) continue;
        const uint8_t *row = ix->row(r);
        for (uint64_t c = 0; c < ix->n_cols; c++)
            if (row[c >> 3] & (0x80u >> (c & 7))) out[c]++;
    }
    return BIGSI_OK;
}

// Pairwise popcounts: per row, the selected A columns that are set, each against every selected B column -- the plain loop
int bigsi_cpu_pairwise_popcounts(bigsi_cpu_index *ix, const uint32_t *cols_a, uint64_t na, const uint32_t *cols_b, uint64_t nb, uint64_t *out,
                                 uint64_t capacity)
{
    if (!ix || !cols_a || !out) return fail(BIGSI_ERR_INVALID, "NULL argument");
    if (na == 0 || (cols_b && nb == 0)) return fail(BIGSI_ERR_INVALID, "an empty list of columns");
    const uint32_t *cb = cols_b ? cols_b : cols_a;
    if (!cols_b) nb = na;
    for (uint64_t i = 0; i < na; i++)
        if (cols_a[i] >= ix->n_cols)
            return fail(BIGSI_ERR_RANGE, "cols_a[%llu] = %u is not a column of the index [0,%llu)", (unsigned long long)i, cols_a[i], (unsigned long long)ix->n_cols);
    for (uint64_t j = 0; cols_b && j < nb; j++)
        if (cols_b[j] >= ix->n_cols)
            return fail(BIGSI_ERR_RANGE, "cols_b[%llu] = %u is not a column of the index [0,%llu)", (unsigned long long)j, cols_b[j], (unsigned long long)ix->n_cols);
    const unsigned __int128 pairs = (unsigned __int128)na * nb;
    if (pairs > capacity) return fail(BIGSI_ERR_CAPACITY, "capacity %llu is below na x nb = %llu x %llu", (unsigned long long)capacity, (unsigned long long)na, (unsigned long long)nb);
    if (pairs > BIGSI_PAIRWISE_MAX_PAIRS)
        return fail(BIGSI_ERR_RANGE, "na x nb = %llu x %llu is above BIGSI_PAIRWISE_MAX_PAIRS (%llu)", (unsigned long long)na, (unsigned long long)nb, (unsigned long long)BIGSI_PAIRWISE_MAX_PAIRS);
    TRY(read_only(ix));
    for (uint64_t e = 0; e < na * nb; e++) out[e] = 0;
    for (uint64_t r = 0; r < ix->m; r++) {
        const uint8_t *row = ix->row(r);
        for (uint64_t i = 0; i < na; i++) {
            if (!(row[cols_a[i] >> 3] & (0x80u >> (cols_a[i] & 7)))) continue;
            for (uint64_t j = 0; j < nb; j++)
                if (row[cb[j] >> 3] & (0x80u >> (cb[j] & 7))) out[i * nb + j]++;
        }
    }
    return BIGSI_OK;
}

// the kept columns of a row, in order, closed up: one bit at a time (dst and src may be the same row: column j is written after
// column >= j was read)
static uint64_t select_columns(uint8_t *dst, uint64_t dst_stride, const uint8_t *src, uint64_t n_cols, const uint8_t *keep)
{
    uint64_t j = 0;
    for (uint64_t c = 0; c < n_cols; c++) {
        if (!(keep[c >> 3] & (0x80u >> (c & 7)))) continue;
        const bool on = src[c >> 3] & (0x80u >> (c & 7));
        const uint8_t mask = (uint8_t)(0x80u >> (j & 7));
        if (on) dst[j >> 3] |= mask;
        else dst[j >> 3] &= (uint8_t)~mask;
        j++;
    }
    for (uint64_t c = j; c < dst_stride * 8 && (c & 7); c++) dst[c >> 3] &= (uint8_t)~(0x80u >> (c & 7));
    memset(dst + ceil_div(j, 8), 0, dst_stride - ceil_div(j, 8));
    return j;
}

int bigsi_cpu_compact_columns(bigsi_cpu_index *ix, const uint8_t *keep, uint64_t *new_num_cols)
{
    TRY(read_only(ix));
    if (!ix || !keep) return fail(BIGSI_ERR_INVALID, "NULL argument");
    uint64_t kept = 0;
    for (uint64_t c = 0; c < ix->n_cols; c++) kept += (keep[c >> 3] & (0x80u >> (c & 7))) ? 1 : 0;
    if (kept < ix->n_cols) {          // (every column kept: the rows stay as they are)
        for (uint64_t r = 0; r < ix->m; r++) select_columns(ix->row(r), ix->stride, ix->row(r), ix->n_cols, keep);
        ix->n_cols = kept;
    }
    if (new_num_cols) *new_num_cols = kept;
    return BIGSI_OK;
}

int bigsi_cpu_extract_columns(bigsi_cpu_index *dst, const bigsi_cpu_index *src, const uint8_t *keep)
{
    if (!keep) return fail(BIGSI_ERR_INVALID, "NULL argument");
    TRY(check_derive({/*in_place*/ "bigsi_cpu_compact_columns", /*rows_divide*/ false, /*same_hashes*/ false}, dst, src));
    uint64_t kept = 0;
    for (uint64_t c = 0; c < src->n_cols; c++) kept += (keep[c >> 3] & (0x80u >> (c & 7))) ? 1 : 0;
    TRY(bigsi_cpu_reserve_cols(dst, kept));
    std::vector<uint8_t> tmp, page;
    const uint64_t rb = src->rb();
    for (uint64_t r = 0; r < src->m; r++) select_columns(dst->row(r), dst->stride, src->fetch(r, rb, tmp, page), src->n_cols, keep);
    dst->n_cols = kept;
    return bdb_read_failed(src);
}

// Column collapse: destination column g = the OR of the source columns of group g, one row and one column at a time
int bigsi_cpu_collapse_columns_into(bigsi_cpu_index *dst, const bigsi_cpu_index *src, const uint32_t *group_of, uint64_t num_groups)
{
    if (!dst || !src || !group_of) return fail(BIGSI_ERR_INVALID, "NULL argument");
    if (num_groups == 0 || num_groups >= 0xFFFFFFFFull) return fail(BIGSI_ERR_INVALID, "num_groups %llu is not in [1, 2^32 - 1)", (unsigned long long)num_groups);
    TRY(check_derive({/*in_place*/ nullptr, /*rows_divide*/ false, /*same_hashes*/ true}, dst, src));
    for (uint64_t c = 0; c < src->n_cols; c++)
        if (group_of[c] != BIGSI_COLLAPSE_DROPPED && group_of[c] >= num_groups)
            return fail(BIGSI_ERR_INVALID, "group_of[%llu] = %u is neither a group id below %llu nor BIGSI_COLLAPSE_DROPPED", (unsigned long long)c, group_of[c],
                        (unsigned long long)num_groups);
    TRY(bigsi_cpu_reserve_cols(dst, num_groups));
    std::vector<uint8_t> tmp, page;
    const uint64_t rb = src->rb();
    for (uint64_t r = 0; r < src->m; r++) {
        const uint8_t *x = src->fetch(r, rb, tmp, page);
        uint8_t *y = dst->row(r);
        memset(y, 0, dst->stride);
        for (uint64_t c = 0; c < src->n_cols; c++) {
            const uint32_t g = group_of[c];
            if (g != BIGSI_COLLAPSE_DROPPED && (x[c >> 3] & (0x80u >> (c & 7)))) y[g >> 3] |= (uint8_t)(0x80u >> (g & 7));
        }
    }
    dst->n_cols = num_groups;
    return bdb_read_failed(src);
}

// Consensus collapse: destination column g = 1 where at least min_members[g] source columns of group g are set, one row and one
// column at a time, one counter per group
int bigsi_cpu_consensus_columns_into(bigsi_cpu_index *dst, const bigsi_cpu_index *src, const uint32_t *group_of, uint64_t num_groups,
                                     const uint32_t *min_members)
{
    if (!dst || !src || !group_of || !min_members) return fail(BIGSI_ERR_INVALID, "NULL argument");
    if (num_groups == 0 || num_groups >= 0xFFFFFFFFull) return fail(BIGSI_ERR_INVALID, "num_groups %llu is not in [1, 2^32 - 1)", (unsigned long long)num_groups);
    TRY(check_derive({/*in_place*/ nullptr, /*rows_divide*/ false, /*same_hashes*/ true}, dst, src));
    for (uint64_t c = 0; c < src->n_cols; c++)
        if (group_of[c] != BIGSI_COLLAPSE_DROPPED && group_of[c] >= num_groups)
            return fail(BIGSI_ERR_INVALID, "group_of[%llu] = %u is neither a group id below %llu nor BIGSI_COLLAPSE_DROPPED", (unsigned long long)c, group_of[c],
                        (unsigned long long)num_groups);
    for (uint64_t g = 0; g < num_groups; g++)
        if (min_members[g] == 0)
            return fail(BIGSI_ERR_INVALID, "min_members[%llu] is 0: a group keeps a bit that at least one member has (0 would mean an all-ones column)",
                        (unsigned long long)g);
    TRY(bigsi_cpu_reserve_cols(dst, num_groups));
    std::vector<uint8_t> tmp, page;
    std::vector<uint64_t> count(num_groups);
    const uint64_t rb = src->rb();
    for (uint64_t r = 0; r < src->m; r++) {
        const uint8_t *x = src->fetch(r, rb, tmp, page);
        uint8_t *y = dst->row(r);
        memset(y, 0, dst->stride);
        std::fill(count.begin(), count.end(), 0ull);
        for (uint64_t c = 0; c < src->n_cols; c++) {
            const uint32_t g = group_of[c];
            if (g != BIGSI_COLLAPSE_DROPPED && (x[c >> 3] & (0x80u >> (c & 7)))) count[g]++;
        }
        for (uint64_t g = 0; g < num_groups; g++)
            if (count[g] >= min_members[g]) y[g >> 3] |= (uint8_t)(0x80u >> (g & 7));
    }
    dst->n_cols = num_groups;
    return bdb_read_failed(src);
}

// row r of the folded matrix: the OR of the source rows r, r + m_dst, ..., r + (factor - 1) m_dst over the bytes that carry columns,
// the bits behind the last column cleared and the rest of the destination stride zeroed (dst may be the source's own row r: the j = 0
// term is read before the row is written)
static void fold_row(uint8_t *dst, uint64_t dst_stride, const bigsi_cpu_index *src, uint64_t r, uint64_t m_dst, uint64_t factor,
                     std::vector<uint8_t> &acc, std::vector<uint8_t> &tmp, std::vector<uint8_t> &page)
{
    const uint64_t rb = src->rb();
    acc.assign(rb, 0);
    for (uint64_t j = 0; j < factor; j++) {
        const uint8_t *x = src->fetch(r + j * m_dst, rb, tmp, page);
        for (uint64_t b = 0; b < rb; b++) acc[b] |= x[b];
    }
    if (src->n_cols & 7) acc[rb - 1] &= (uint8_t)(0xFF00u >> (src->n_cols & 7));
    memcpy(dst, acc.data(), rb);
    memset(dst + rb, 0, dst_stride - rb);
}

int bigsi_cpu_fold_rows(bigsi_cpu_index *ix, uint64_t factor, uint64_t *new_num_rows)
{
    TRY(read_only(ix));
    if (!ix) return fail(BIGSI_ERR_INVALID, "NULL index");
    if (factor == 0 || ix->m % factor)
        return fail(BIGSI_ERR_INVALID, "fold factor %llu does not divide num_rows %llu", (unsigned long long)factor, (unsigned long long)ix->m);
    if (factor > 1) {
        const uint64_t m_dst = ix->m / factor;
        std::vector<uint8_t> acc, tmp, page;
        for (uint64_t r = 0; r < m_dst; r++) fold_row(ix->row(r), ix->stride, ix, r, m_dst, factor, acc, tmp, page);
        ix->m = m_dst;          // (the table keeps its size until bigsi_cpu_trim_rows)
    }
    if (new_num_rows) *new_num_rows = ix->m;
    return BIGSI_OK;
}

int bigsi_cpu_fold_rows_into(bigsi_cpu_index *dst, const bigsi_cpu_index *src)
{
    TRY(check_derive({/*in_place*/ "bigsi_cpu_fold_rows", /*rows_divide*/ true, /*same_hashes*/ true}, dst, src));
    TRY(bigsi_cpu_reserve_cols(dst, src->n_cols));
    std::vector<uint8_t> acc, tmp, page;
    const uint64_t factor = src->m / dst->m;
    for (uint64_t r = 0; r < dst->m; r++) fold_row(dst->row(r), dst->stride, src, r, dst->m, factor, acc, tmp, page);
    dst->n_cols = src->n_cols;
    return bdb_read_failed(src);
}

int bigsi_cpu_trim_rows(bigsi_cpu_index *ix)
{
    TRY(read_only(ix));
    if (!ix) return fail(BIGSI_ERR_INVALID, "NULL index");
    if (ix->alloc_rows <= ix->m) return BIGSI_OK;
    uint8_t *kept = static_cast<uint8_t *>(malloc(std::max<uint64_t>(ix->m * ix->stride, 1)));
    if (!kept) return fail(BIGSI_ERR_NOMEM, "cannot allocate %llu x %llu bytes", (unsigned long long)ix->m, (unsigned long long)ix->stride);
    memcpy(kept, ix->rows, ix->m * ix->stride);
    free(ix->rows);
    ix->rows = kept;
    ix->alloc_rows = ix->m;
    return BIGSI_OK;
}

int bigsi_cpu_insert_kmers(bigsi_cpu_index *ix, uint64_t col, const char *seqs, const uint64_t *offsets, uint32_t n_seqs, uint32_t k)
{
    TRY(read_only(ix));
    if (!ix) return fail(BIGSI_ERR_INVALID, "NULL index");
    if (n_seqs == 0) return BIGSI_OK;
    TRY(check_seqs(seqs, offsets, n_seqs, k));
    if (col >= ix->n_cols) return fail(BIGSI_ERR_RANGE, "column %llu out of range (num_cols %llu)", (unsigned long long)col, (unsigned long long)ix->n_cols);
    std::string canon;
    std::vector<uint64_t> r(ix->h);
    for (uint32_t i = 0; i < n_seqs; i++) {
        const char *s = seqs + offsets[i];
        const uint64_t len = offsets[i + 1] - offsets[i];
        for (uint64_t p = 0; p + k <= len; p++) {
            canonical(s + p, k, canon);
            rows_of(canon, ix->h, ix->m, r.data());
            for (uint32_t t = 0; t < ix->h; t++) ix->row(r[t])[col >> 3] |= (uint8_t)(0x80u >> (col & 7));
        }
    }
    return BIGSI_OK;
}

int bigsi_cpu_fill_synthetic(bigsi_cpu_index *ix, uint64_t seed, uint64_t shard, uint32_t and_draws)
{
    TRY(read_only(ix));
    if (!ix) return fail(BIGSI_ERR_INVALID, "NULL index");
    const uint64_t base = mix64(seed + shard * 0x632BE59BD9B4E019ull), words = ix->stride / 8;
    for (uint64_t r = 0; r < ix->m; r++) {
        const uint64_t rk = mix64(base ^ (r * 0x9E3779B97F4A7C15ull));
        for (uint64_t w = 0; w < words; w++) {
            uint64_t v = ~0ull;
            for (uint32_t d = 0; d < and_draws; d++) v &= mix64(rk + (w * 8 + d) * 0xD1B54A32D192ED03ull);
            v &= valid_word_mask(w, ix->n_cols);
            memcpy(ix->row(r) + 8 * w, &v, 8);
        }
    }
    return BIGSI_OK;
}

int bigsi_cpu_bloom(int, const char *kmers, uint64_t u, uint32_t k, uint64_t m, uint32_t h, uint32_t flags, uint8_t *out)
{
    if (!out || (u && !kmers)) return fail(BIGSI_ERR_INVALID, "NULL argument");
    if (k == 0 || m == 0 || h == 0) return fail(BIGSI_ERR_INVALID, "k, m and h must be > 0");
    memset(out, 0, ceil_div(m, 8));
    std::string canon;
    std::vector<uint64_t> r(h);
    for (uint64_t i = 0; i < u; i++) {
        if (flags & BIGSI_BLOOM_RAW) canon.assign(kmers + i * k, k);
        else canonical(kmers + i * k, k, canon);
        rows_of(canon, h, m, r.data());
        for (uint32_t t = 0; t < h; t++) out[r[t] >> 3] |= (uint8_t)(0x80u >> (r[t] & 7));
    }
    return BIGSI_OK;
}

int bigsi_cpu_lookup(bigsi_cpu_index *ix, const char *kmers, uint32_t k, uint64_t u, uint8_t *out_rows)
{
    if (!ix || (u && (!kmers || !out_rows))) return fail(BIGSI_ERR_INVALID, "NULL argument");
    if (k == 0) return fail(BIGSI_ERR_INVALID, "k must be > 0");
    if (u == 0) return BIGSI_OK;
    if (ix->n_cols == 0) return fail(BIGSI_ERR_STATE, "index has no columns");
    const uint64_t rb = ix->rb();
    std::string canon;
    std::vector<uint64_t> r(ix->h);
    std::vector<uint8_t> tmp, page;
    for (uint64_t i = 0; i < u; i++) {
        canonical(kmers + i * k, k, canon);
        rows_of(canon, ix->h, ix->m, r.data());
        uint8_t *o = out_rows + i * rb;
        memcpy(o, ix->fetch(r[0], rb, tmp, page), rb);
        for (uint32_t t = 1; t < ix->h; t++) {
            const uint8_t *x = ix->fetch(r[t], rb, tmp, page);
            for (uint64_t b = 0; b < rb; b++) o[b] &= x[b];
        }
    }
    return bdb_read_failed(ix);
}

int bigsi_cpu_search_stream(bigsi_cpu_index *ix, const char *seqs, const uint64_t *offsets, uint64_t n_seqs, uint32_t k,
                            double threshold, uint32_t flags, uint32_t *num_kmers, uint32_t *num_unique, uint32_t *min_kmers,
                            uint64_t *hit_offsets, uint32_t *colours, uint32_t *counts, uint64_t hit_capacity)
{
    if (!hit_offsets) return fail(BIGSI_ERR_INVALID, "hit_offsets is NULL");
    if (!ix) return fail(BIGSI_ERR_INVALID, "NULL index");
    TRY(check_seqs(seqs, offsets, n_seqs, k));
    if (!(threshold <= 1.0)) return fail(BIGSI_ERR_INVALID, "threshold must be <= 1 (bigsi/graph/bigsi.py:176), got %g", threshold);
    if (ix->n_cols == 0) return fail(BIGSI_ERR_STATE, "index has no columns");
    if (ix->bdb && (flags & BIGSI_CPU_WORD_PARALLEL)) return fail(BIGSI_ERR_STATE, "BIGSI_CPU_WORD_PARALLEL works on rows resident in RAM, not on a BerkeleyDB-backed index");
    Hits hits{hit_offsets, colours, counts, hit_capacity};
    QueryKmers q;
    for (uint64_t i = 0; i < n_seqs; i++) {
        uint32_t nk, nu, mk;
        hit_offsets[i] = hits.total;
        if (flags & BIGSI_CPU_WORD_PARALLEL) search_word_parallel(ix, seqs + offsets[i], offsets[i + 1] - offsets[i], k, threshold, q, &nk, &nu, &mk, hits);
        else search_reference_shaped(ix, seqs + offsets[i], offsets[i + 1] - offsets[i], k, threshold, q, &nk, &nu, &mk, hits);
        if (num_kmers) num_kmers[i] = nk;
        if (num_unique) num_unique[i] = nu;
        if (min_kmers) min_kmers[i] = mk;
    }
    hit_offsets[n_seqs] = hits.total;
    TRY(bdb_read_failed(ix));
    if (hits.total > hit_capacity)
        return fail(BIGSI_ERR_CAPACITY, "hit buffers hold %llu entries, %llu needed", (unsigned long long)hit_capacity, (unsigned long long)hits.total);
    return BIGSI_OK;
}

int bigsi_cpu_search_batch(bigsi_cpu_index *ix, const char *seqs, const uint64_t *offsets, uint32_t n_seqs, uint32_t k,
                           double threshold, uint32_t flags, uint32_t *num_kmers, uint32_t *num_unique, uint32_t *min_kmers,
                           uint64_t *hit_offsets, uint32_t *colours, uint32_t *counts, uint64_t hit_capacity)
{
    return bigsi_cpu_search_stream(ix, seqs, offsets, n_seqs, k, threshold, flags, num_kmers, num_unique, min_kmers, hit_offsets, colours, counts, hit_capacity);
}

int bigsi_cpu_presence(bigsi_cpu_index *ix, const char *seq, uint64_t len, uint32_t k, const uint32_t *colours, uint32_t n_colours, uint8_t *out)
{
    if (!ix || (len && !seq)) return fail(BIGSI_ERR_INVALID, "NULL argument");
    if (k == 0) return fail(BIGSI_ERR_INVALID, "k must be > 0");
    if (n_colours == 0 || len < k) return BIGSI_OK;
    if (!colours || !out) return fail(BIGSI_ERR_INVALID, "NULL argument");
    for (uint32_t j = 0; j < n_colours; j++)
        if (colours[j] >= ix->n_cols) return fail(BIGSI_ERR_RANGE, "colour %u >= num_cols", colours[j]);
    const uint64_t n = len - k + 1;
    std::string canon;
    std::vector<uint64_t> r(ix->h);
    std::vector<uint8_t> tmp, page;
    for (uint64_t i = 0; i < n; i++) {
        canonical(seq + i, k, canon);
        rows_of(canon, ix->h, ix->m, r.data());
        for (uint32_t j = 0; j < n_colours; j++) {
            const uint32_t c = colours[j];
            bool present = true;
            for (uint32_t t = 0; t < ix->h && present; t++) present = (ix->fetch(r[t], ix->rb(), tmp, page)[c >> 3] & (0x80u >> (c & 7))) != 0;
            out[(uint64_t)j * n + i] = present ? '1' : '0';
        }
    }
    return bdb_read_failed(ix);
}

// per k-mer position the number of samples that hold the k-mer: every unique k-mer string of a sequence is swept once (the AND of
// its h rows, byte by byte, under the universe and the subset masks, the bits behind the last column cut off) and the two numbers are
// expanded over the positions that carry it
int bigsi_cpu_kmer_prevalence(bigsi_cpu_index *ix, const char *seqs, const uint64_t *offsets, uint32_t n_seqs, uint32_t k,
                              const uint8_t *universe, const uint8_t *subset, uint64_t *pos_offsets, uint32_t *total, uint32_t *in_subset,
                              uint64_t capacity)
{
    if (!ix) return fail(BIGSI_ERR_INVALID, "NULL argument");
    TRY(check_seqs(seqs, offsets, n_seqs, k));
    if (!pos_offsets) return fail(BIGSI_ERR_INVALID, "pos_offsets is NULL");
    if (!total) return fail(BIGSI_ERR_INVALID, "total is NULL");
    if (in_subset && !subset) return fail(BIGSI_ERR_INVALID, "in_subset given without a subset mask");
    if (subset && !in_subset) return fail(BIGSI_ERR_INVALID, "a subset mask given without in_subset");
    pos_offsets[0] = 0;
    for (uint32_t i = 0; i < n_seqs; i++) {
        const uint64_t len = offsets[i + 1] - offsets[i];
        pos_offsets[i + 1] = pos_offsets[i] + (len >= k ? len - k + 1 : 0);
    }
    if (capacity < pos_offsets[n_seqs])
        return fail(BIGSI_ERR_CAPACITY, "prevalence buffers hold %llu entries, %llu needed", (unsigned long long)capacity, (unsigned long long)pos_offsets[n_seqs]);
    if (ix->n_cols == 0) return fail(BIGSI_ERR_STATE, "index has no columns");
    const uint64_t rb = ix->rb();
    const uint8_t last = (ix->n_cols & 7) ? (uint8_t)(0xFF00u >> (ix->n_cols & 7)) : (uint8_t)0xFF;
    QueryKmers q;
    std::string canon;
    std::vector<uint64_t> r(ix->h);
    std::vector<uint8_t> acc(rb), tmp, page;
    std::vector<uint32_t> n_all, n_sub;
    for (uint32_t i = 0; i < n_seqs; i++) {
        const char *s = seqs + offsets[i];
        unique_kmers(s, offsets[i + 1] - offsets[i], k, q);
        n_all.assign(q.first_pos.size(), 0);
        n_sub.assign(q.first_pos.size(), 0);
        for (size_t j = 0; j < q.first_pos.size(); j++) {
            canonical(s + q.first_pos[j], k, canon);
            rows_of(canon, ix->h, ix->m, r.data());
            std::fill(acc.begin(), acc.end(), 0xFF);
            for (uint32_t t = 0; t < ix->h; t++) {
                const uint8_t *x = ix->fetch(r[t], rb, tmp, page);
                for (uint64_t b = 0; b < rb; b++) acc[b] &= x[b];
            }
            acc[rb - 1] &= last;
            for (uint64_t b = 0; b < rb; b++) {
                const uint8_t a = universe ? (uint8_t)(acc[b] & universe[b]) : acc[b];
                n_all[j] += (uint32_t)__builtin_popcount(a);
                if (subset) n_sub[j] += (uint32_t)__builtin_popcount(a & subset[b]);
            }
        }
        for (size_t p = 0; p < q.pos_unique.size(); p++) {
            total[pos_offsets[i] + p] = n_all[q.pos_unique[p]];
            if (subset) in_subset[pos_offsets[i] + p] = n_sub[q.pos_unique[p]];
        }
    }
    return bdb_read_failed(ix);
}

// the windowed search (include/bigsi_cpu_window.h): per sequence a plain loop over the positions -- the AND of the position's h rows,
// the bits behind the last column cut off -- that keeps, per column, the prefix sum of its presence; then per column the window
// differences pre[s + We] - pre[s] over the starts: the maximum and its lowest start, the first and last start that reach `need`
// and their number.  Columns in ascending order, so the hits are.
int bigsi_cpu_window_search(bigsi_cpu_index *ix, const char *seqs, const uint64_t *offsets, uint32_t n_seqs, uint32_t k, uint32_t window,
                            double threshold, uint32_t *window_used, uint32_t *need, uint64_t *hit_offsets, uint32_t *colours,
                            bigsi_hip_window_hit *records, uint64_t capacity)
{
    if (!ix) return fail(BIGSI_ERR_INVALID, "NULL argument");
    TRY(check_seqs(seqs, offsets, n_seqs, k));
    if (window == 0 || window > BIGSI_WINDOW_MAX) return fail(BIGSI_ERR_INVALID, "window must be 1 .. %u k-mer positions (got %u)", BIGSI_WINDOW_MAX, window);
    if (!(threshold > 0.0 && threshold <= 1.0)) return fail(BIGSI_ERR_INVALID, "threshold must be in (0, 1] (got %g)", threshold);
    if (!window_used || !need || !hit_offsets) return fail(BIGSI_ERR_INVALID, "window_used, need or hit_offsets is NULL");
    if (capacity && (!colours || !records)) return fail(BIGSI_ERR_INVALID, "colours or records is NULL");
    if (ix->n_cols == 0) return fail(BIGSI_ERR_STATE, "index has no columns");
    const uint64_t rb = ix->rb(), n_cols = ix->n_cols;
    std::string canon;
    std::vector<uint64_t> r(ix->h);
    std::vector<uint8_t> acc(rb), tmp, page;
    std::vector<uint32_t> pre;                      // pre[p * n_cols + c]: positions < p that hold column c
    std::vector<uint32_t> out_col;
    std::vector<bigsi_hip_window_hit> out_rec;
    hit_offsets[0] = 0;
    for (uint32_t i = 0; i < n_seqs; i++) {
        const char *s = seqs + offsets[i];
        const uint64_t len = offsets[i + 1] - offsets[i], n = len >= k ? len - k + 1 : 0;
        const uint32_t we = (uint32_t)std::min<uint64_t>(n, window), thr = (uint32_t)ceil((double)we * threshold);
        window_used[i] = we;
        need[i] = thr;
        if (n) {
            pre.assign((n + 1) * n_cols, 0);
            for (uint64_t p = 0; p < n; p++) {
                canonical(s + p, k, canon);
                rows_of(canon, ix->h, ix->m, r.data());
                std::fill(acc.begin(), acc.end(), 0xFF);
                for (uint32_t t = 0; t < ix->h; t++) {
                    const uint8_t *x = ix->fetch(r[t], rb, tmp, page);
                    for (uint64_t b = 0; b < rb; b++) acc[b] &= x[b];
                }
                for (uint64_t c = 0; c < n_cols; c++)
                    pre[(p + 1) * n_cols + c] = pre[p * n_cols + c] + ((acc[c >> 3] & (0x80u >> (c & 7))) ? 1u : 0u);
            }
            const uint64_t starts = n - we + 1;
            for (uint64_t c = 0; c < n_cols; c++) {
                bigsi_hip_window_hit h{0, 0, 0, 0, 0, 0};
                for (uint64_t st = 0; st < starts; st++) {
                    const uint32_t found = pre[(st + we) * n_cols + c] - pre[st * n_cols + c];
                    if (st == 0 || found > h.best_found) { h.best_found = found; h.best_start = (uint32_t)st; }
                    if (found >= thr) {
                        if (!h.windows_passing) h.first_start = (uint32_t)st;
                        h.last_start = (uint32_t)st;
                        h.windows_passing++;
                    }
                }
                if (h.windows_passing) { out_col.push_back((uint32_t)c); out_rec.push_back(h); }
            }
        }
        hit_offsets[i + 1] = out_col.size();
    }
    TRY(bdb_read_failed(ix));
    if (out_col.size() > capacity)
        return fail(BIGSI_ERR_CAPACITY, "hit buffers hold %llu entries, %llu needed", (unsigned long long)capacity, (unsigned long long)out_col.size());
    if (!out_col.empty()) {
        memcpy(colours, out_col.data(), out_col.size() * 4);
        memcpy(records, out_rec.data(), out_rec.size() * sizeof(bigsi_hip_window_hit));
    }
    return BIGSI_OK;
}

// the query-set tally: every sequence searched in the reference's shape (search_reference_shaped: its hits are the (sample, k-mers
// found) pairs a search reports), a sequence without k-mers skipped, the hits summed per sample.  A threshold below 0 asks for what 0
// asks for (min_kmers is clamped at 0: every sample passes).
int bigsi_cpu_search_tally(bigsi_cpu_index *ix, const char *seqs, const uint64_t *offsets, uint64_t n_seqs, uint32_t k, double threshold,
                           uint64_t *queries_hit, uint64_t *kmers_found, uint64_t capacity, uint64_t totals[4])
{
    if (!ix || !queries_hit || !kmers_found || !totals) return fail(BIGSI_ERR_INVALID, "NULL argument");
    TRY(check_seqs(seqs, offsets, n_seqs, k));
    if (!(threshold <= 1.0)) return fail(BIGSI_ERR_INVALID, "threshold must be <= 1, got %g", threshold);
    if (capacity < ix->n_cols)
        return fail(BIGSI_ERR_CAPACITY, "tally buffers hold %llu entries, %llu needed", (unsigned long long)capacity, (unsigned long long)ix->n_cols);
    if (ix->n_cols == 0) return fail(BIGSI_ERR_STATE, "index has no columns");
    const uint64_t n_cols = ix->n_cols;
    std::vector<uint64_t> hit(n_cols, 0), found(n_cols, 0);
    std::vector<uint32_t> col(n_cols), cnt(n_cols);
    uint64_t tot[4] = {0, 0, 0, 0};
    QueryKmers q;
    for (uint64_t i = 0; i < n_seqs; i++) {
        uint32_t nk, nu, mk;
        Hits hits{nullptr, col.data(), cnt.data(), n_cols};
        search_reference_shaped(ix, seqs + offsets[i], offsets[i + 1] - offsets[i], k, threshold < 0.0 ? 0.0 : threshold, q, &nk, &nu, &mk, hits);
        if (nu == 0) { tot[2]++; continue; }
        tot[0]++;
        tot[1] += nu;
        if (hits.total) tot[3]++;
        for (uint64_t j = 0; j < hits.total; j++) {
            hit[col[j]]++;
            found[col[j]] += cnt[j];
        }
    }
    TRY(bdb_read_failed(ix));
    memcpy(queries_hit, hit.data(), n_cols * 8);
    memcpy(kmers_found, found.data(), n_cols * 8);
    memcpy(totals, tot, sizeof tot);
    return BIGSI_OK;
}

// read classification: every sequence searched in the reference's shape, its hits (ascending colours, each with the k-mers found)
// weighed per group -- the number of hit columns, the largest count and the first colour that holds it --, then the two best hit
// groups by (found descending, lower id).  A threshold below 0 asks for what 0 asks for.
int bigsi_cpu_classify(bigsi_cpu_index *ix, const char *seqs, const uint64_t *offsets, uint64_t n_seqs, uint32_t k, double threshold,
                       const uint32_t *group_of, uint64_t n_entries, uint32_t n_groups, bigsi_hip_classify_record *records)
{
    if (!ix || !group_of || !records) return fail(BIGSI_ERR_INVALID, "NULL argument");
    TRY(check_seqs(seqs, offsets, n_seqs, k));
    if (!(threshold <= 1.0)) return fail(BIGSI_ERR_INVALID, "threshold must be <= 1, got %g", threshold);
    if (ix->n_cols == 0) return fail(BIGSI_ERR_STATE, "index has no columns");
    if (n_entries != ix->n_cols)
        return fail(BIGSI_ERR_INVALID, "group_of has %llu entries, the index has %llu columns", (unsigned long long)n_entries, (unsigned long long)ix->n_cols);
    if (n_groups == 0 || n_groups > BIGSI_CLASSIFY_MAX_GROUPS) return fail(BIGSI_ERR_INVALID, "n_groups must be 1 .. %u (got %u)", BIGSI_CLASSIFY_MAX_GROUPS, n_groups);
    for (uint64_t c = 0; c < n_entries; c++)
        if (group_of[c] != BIGSI_CLASSIFY_NONE && group_of[c] >= n_groups)
            return fail(BIGSI_ERR_INVALID, "group_of[%llu] = %u is neither below n_groups (%u) nor BIGSI_CLASSIFY_NONE", (unsigned long long)c, group_of[c], n_groups);
    const uint64_t n_cols = ix->n_cols;
    std::vector<uint32_t> col(n_cols), cnt(n_cols), samples(n_groups), found(n_groups), colour(n_groups);
    std::vector<bigsi_hip_classify_record> out(n_seqs);
    QueryKmers q;
    for (uint64_t i = 0; i < n_seqs; i++) {
        uint32_t nk, nu, mk;
        Hits hits{nullptr, col.data(), cnt.data(), n_cols};
        search_reference_shaped(ix, seqs + offsets[i], offsets[i + 1] - offsets[i], k, threshold < 0.0 ? 0.0 : threshold, q, &nk, &nu, &mk, hits);
        bigsi_hip_classify_record r = {0, 0, 0, 0, BIGSI_CLASSIFY_NONE, 0, BIGSI_CLASSIFY_NONE, 0, BIGSI_CLASSIFY_NONE, 0, BIGSI_CLASSIFY_NONE, 0};
        if (nu) {
            r.num_unique = nu;
            r.min_kmers = mk;
            std::fill(samples.begin(), samples.end(), 0u);
            for (uint64_t j = 0; j < hits.total; j++) {
                const uint32_t g = group_of[col[j]];
                if (g == BIGSI_CLASSIFY_NONE) continue;
                r.samples_hit++;
                if (samples[g]++ == 0 || cnt[j] > found[g]) { found[g] = cnt[j]; colour[g] = col[j]; }
            }
            for (uint32_t g = 0; g < n_groups; g++) {
                if (!samples[g]) continue;
                r.groups_hit++;
                if (r.best_group == BIGSI_CLASSIFY_NONE || found[g] > r.best_found) {
                    r.second_group = r.best_group; r.second_found = r.best_found; r.second_colour = r.best_colour; r.second_samples_hit = r.best_samples_hit;
                    r.best_group = g; r.best_found = found[g]; r.best_colour = colour[g]; r.best_samples_hit = samples[g];
                } else if (r.second_group == BIGSI_CLASSIFY_NONE || found[g] > r.second_found) {
                    r.second_group = g; r.second_found = found[g]; r.second_colour = colour[g]; r.second_samples_hit = samples[g];
                }
            }
        }
        out[i] = r;
    }
    TRY(bdb_read_failed(ix));
    memcpy(records, out.data(), n_seqs * sizeof(bigsi_hip_classify_record));
    return BIGSI_OK;
}

// group association: every sequence searched in the reference's shape, then a loop over its hit columns (ascending colours): one more
// sample hit, and one more for the column's group when it has one.  A threshold below 0 asks for what 0 asks for.
int bigsi_cpu_associate(bigsi_cpu_index *ix, const char *seqs, const uint64_t *offsets, uint64_t n_seqs, uint32_t k, double threshold,
                        const uint32_t *group_of, uint64_t n_entries, uint32_t n_groups, uint32_t *counts, bigsi_hip_associate_info *info)
{
    if (!ix || !group_of || !counts || !info) return fail(BIGSI_ERR_INVALID, "NULL argument");
    TRY(check_seqs(seqs, offsets, n_seqs, k));
    if (!(threshold <= 1.0)) return fail(BIGSI_ERR_INVALID, "threshold must be <= 1, got %g", threshold);
    if (ix->n_cols == 0) return fail(BIGSI_ERR_STATE, "index has no columns");
    if (n_entries != ix->n_cols)
        return fail(BIGSI_ERR_INVALID, "group_of has %llu entries, the index has %llu columns", (unsigned long long)n_entries, (unsigned long long)ix->n_cols);
    if (n_groups == 0 || n_groups > BIGSI_ASSOCIATE_MAX_GROUPS) return fail(BIGSI_ERR_INVALID, "n_groups must be 1 .. BIGSI_ASSOCIATE_MAX_GROUPS = %u (got %u)", BIGSI_ASSOCIATE_MAX_GROUPS, n_groups);
    for (uint64_t c = 0; c < n_entries; c++)
        if (group_of[c] != BIGSI_ASSOCIATE_NONE && group_of[c] >= n_groups)
            return fail(BIGSI_ERR_INVALID, "group_of[%llu] = %u is neither below n_groups (%u) nor BIGSI_ASSOCIATE_NONE", (unsigned long long)c, group_of[c], n_groups);
    const uint64_t n_cols = ix->n_cols;
    std::vector<uint32_t> col(n_cols), cnt(n_cols), out((size_t)n_seqs * n_groups, 0u);
    std::vector<bigsi_hip_associate_info> out_info(n_seqs);
    QueryKmers q;
    for (uint64_t i = 0; i < n_seqs; i++) {
        uint32_t nk, nu, mk;
        Hits hits{nullptr, col.data(), cnt.data(), n_cols};
        search_reference_shaped(ix, seqs + offsets[i], offsets[i + 1] - offsets[i], k, threshold < 0.0 ? 0.0 : threshold, q, &nk, &nu, &mk, hits);
        bigsi_hip_associate_info r = {0, 0, 0, 0};
        if (nu) {
            r.num_unique = nu;
            r.min_kmers = mk;
            for (uint64_t j = 0; j < hits.total; j++) {
                const uint32_t g = group_of[col[j]];
                r.samples_hit++;
                if (g == BIGSI_ASSOCIATE_NONE) continue;
                r.grouped_hit++;
                out[(size_t)i * n_groups + g]++;
            }
        }
        out_info[i] = r;
    }
    TRY(bdb_read_failed(ix));
    memcpy(counts, out.data(), out.size() * sizeof(uint32_t));
    memcpy(info, out_info.data(), n_seqs * sizeof(bigsi_hip_associate_info));
    return BIGSI_OK;
}

// panel genotyping: every probe searched in the reference's shape, then a loop over its hit columns: the column's bit of the probe's
// allele plane is set when the column is selected.  The calls and counts follow column by column, variant by variant, as genotypes()
// of bigsi_amd/variant_search.py takes them.  A threshold below 0 asks for what 0 asks for.
int bigsi_cpu_genotype(bigsi_cpu_index *ix, const char *seqs, const uint64_t *offsets, uint64_t n_seqs, uint32_t k, double threshold,
                       const uint32_t *allele_of, uint32_t n_variants, const uint8_t *columns, uint8_t *ref_planes, uint8_t *alt_planes,
                       uint64_t plane_capacity_bytes, uint32_t *variant_counts, uint32_t *sample_counts, uint64_t sample_capacity, uint32_t *allele_probes)
{
    if (!ix || !allele_of || !variant_counts || !sample_counts || !allele_probes) return fail(BIGSI_ERR_INVALID, "NULL argument");
    TRY(check_seqs(seqs, offsets, n_seqs, k));
    if (!(threshold <= 1.0)) return fail(BIGSI_ERR_INVALID, "threshold must be <= 1, got %g", threshold);
    if (ix->n_cols == 0) return fail(BIGSI_ERR_STATE, "index has no columns");
    if (n_variants == 0 || n_variants > BIGSI_GENOTYPE_MAX_VARIANTS)
        return fail(BIGSI_ERR_INVALID, "n_variants must be 1 .. BIGSI_GENOTYPE_MAX_VARIANTS = %u (got %u)", BIGSI_GENOTYPE_MAX_VARIANTS, n_variants);
    for (uint64_t i = 0; i < n_seqs; i++)
        if (allele_of[i] != BIGSI_GENOTYPE_NONE && allele_of[i] >= 2ull * n_variants)
            return fail(BIGSI_ERR_INVALID, "allele_of[%llu] = %u is neither below 2 x n_variants (%llu) nor BIGSI_GENOTYPE_NONE", (unsigned long long)i, allele_of[i],
                        2ull * n_variants);
    const uint64_t n_cols = ix->n_cols, rb = (n_cols + 7) / 8;
    if (rb > BIGSI_GENOTYPE_PLANE_BYTES / (2ull * n_variants))
        return fail(BIGSI_ERR_NOMEM, "the planes of %u variants over %llu columns take 2 x %u x %llu bytes, above BIGSI_GENOTYPE_PLANE_BYTES = %llu", n_variants,
                    (unsigned long long)n_cols, n_variants, (unsigned long long)rb, (unsigned long long)BIGSI_GENOTYPE_PLANE_BYTES);
    if ((ref_planes || alt_planes) && plane_capacity_bytes < n_variants * rb)
        return fail(BIGSI_ERR_CAPACITY, "a plane buffer holds %llu bytes, %u variants x %llu bytes needed", (unsigned long long)plane_capacity_bytes, n_variants,
                    (unsigned long long)rb);
    if (sample_capacity < n_cols)
        return fail(BIGSI_ERR_CAPACITY, "sample_counts holds %llu entries, %llu needed", (unsigned long long)sample_capacity, (unsigned long long)n_cols);
    auto selected = [&](uint64_t c) { return !columns || ((columns[c >> 3] >> (7 - (c & 7))) & 1u) != 0; };
    std::vector<uint8_t> plane[2] = {std::vector<uint8_t>((size_t)n_variants * rb, 0), std::vector<uint8_t>((size_t)n_variants * rb, 0)};
    std::vector<uint32_t> col(n_cols), cnt(n_cols), used((size_t)n_variants * 2, 0u);
    QueryKmers q;
    for (uint64_t i = 0; i < n_seqs; i++) {
        if (allele_of[i] == BIGSI_GENOTYPE_NONE) continue;
        uint32_t nk, nu, mk;
        Hits hits{nullptr, col.data(), cnt.data(), n_cols};
        search_reference_shaped(ix, seqs + offsets[i], offsets[i + 1] - offsets[i], k, threshold < 0.0 ? 0.0 : threshold, q, &nk, &nu, &mk, hits);
        if (!nu) continue;
        used[allele_of[i]]++;
        uint8_t *row = plane[allele_of[i] & 1u].data() + (size_t)(allele_of[i] >> 1) * rb;
        for (uint64_t j = 0; j < hits.total; j++)
            if (selected(col[j])) row[col[j] >> 3] |= (uint8_t)(0x80u >> (col[j] & 7));
    }
    TRY(bdb_read_failed(ix));
    std::vector<uint32_t> vc((size_t)n_variants * 4, 0u), sc((size_t)n_cols * 2, 0u);
    for (uint32_t v = 0; v < n_variants; v++)
        for (uint64_t c = 0; c < n_cols; c++) {
            if (!selected(c)) continue;
            const bool r = (plane[0][(size_t)v * rb + (c >> 3)] >> (7 - (c & 7))) & 1u, a = (plane[1][(size_t)v * rb + (c >> 3)] >> (7 - (c & 7))) & 1u;
            vc[(size_t)v * 4 + (r ? (a ? 1 : 0) : (a ? 2 : 3))]++;
            sc[c * 2] += a ? 1u : 0u;
            sc[c * 2 + 1] += (r || a) ? 1u : 0u;
        }
    if (ref_planes) memcpy(ref_planes, plane[0].data(), plane[0].size());
    if (alt_planes) memcpy(alt_planes, plane[1].data(), plane[1].size());
    memcpy(variant_counts, vc.data(), vc.size() * 4);
    memcpy(sample_counts, sc.data(), sc.size() * 4);
    memcpy(allele_probes, used.data(), used.size() * 4);
    return BIGSI_OK;
}

// locus typing: every record searched in the reference's shape, then a loop over its hit columns: a selected column's cell of the
// record's locus takes the larger key -- floor(count (2^32 - 1) / unique) above the complement of the allele identity, written out
// here on its own -- and one more hit.  The counts follow cell by cell.  A threshold below 0 asks for what 0 asks for.
int bigsi_cpu_typing(bigsi_cpu_index *ix, const char *seqs, const uint64_t *offsets, uint64_t n_seqs, uint32_t k, double threshold,
                     const uint32_t *locus_of, const uint32_t *allele_of, uint32_t n_loci, const uint8_t *columns, uint64_t *best, uint32_t *hits,
                     uint64_t cell_capacity, uint32_t *locus_counts, uint32_t *sample_counts, uint64_t sample_capacity, uint32_t *records)
{
    if (!ix || !locus_of || !allele_of || !locus_counts || !sample_counts || !records) return fail(BIGSI_ERR_INVALID, "NULL argument");
    TRY(check_seqs(seqs, offsets, n_seqs, k));
    if (!(threshold <= 1.0)) return fail(BIGSI_ERR_INVALID, "threshold must be <= 1, got %g", threshold);
    if (ix->n_cols == 0) return fail(BIGSI_ERR_STATE, "index has no columns");
    if (n_loci == 0 || n_loci > BIGSI_TYPING_MAX_LOCI)
        return fail(BIGSI_ERR_INVALID, "n_loci must be 1 .. BIGSI_TYPING_MAX_LOCI = %u (got %u)", BIGSI_TYPING_MAX_LOCI, n_loci);
    for (uint64_t i = 0; i < n_seqs; i++) {
        if (locus_of[i] == BIGSI_TYPING_NONE) continue;
        if (locus_of[i] >= n_loci)
            return fail(BIGSI_ERR_INVALID, "locus_of[%llu] = %u is neither below n_loci (%u) nor BIGSI_TYPING_NONE", (unsigned long long)i, locus_of[i], n_loci);
        if (allele_of[i] > BIGSI_TYPING_MAX_ALLELE)
            return fail(BIGSI_ERR_INVALID, "allele_of[%llu] = %u is above BIGSI_TYPING_MAX_ALLELE = %u", (unsigned long long)i, allele_of[i], BIGSI_TYPING_MAX_ALLELE);
    }
    const uint64_t n_cols = ix->n_cols, wv = (n_cols + 63) / 64;
    if (wv > BIGSI_TYPING_CELL_BYTES / (768ull * n_loci))
        return fail(BIGSI_ERR_NOMEM, "the cells of %u loci over %llu columns take %u x %llu x 64 x 12 bytes, above BIGSI_TYPING_CELL_BYTES = %llu", n_loci,
                    (unsigned long long)n_cols, n_loci, (unsigned long long)wv, (unsigned long long)BIGSI_TYPING_CELL_BYTES);
    if ((best || hits) && cell_capacity < n_loci * n_cols)
        return fail(BIGSI_ERR_CAPACITY, "a cell buffer holds %llu entries, %u loci x %llu columns needed", (unsigned long long)cell_capacity, n_loci,
                    (unsigned long long)n_cols);
    if (sample_capacity < n_cols)
        return fail(BIGSI_ERR_CAPACITY, "sample_counts holds %llu entries, %llu needed", (unsigned long long)sample_capacity, (unsigned long long)n_cols);
    auto selected = [&](uint64_t c) { return !columns || ((columns[c >> 3] >> (7 - (c & 7))) & 1u) != 0; };
    std::vector<uint64_t> top((size_t)n_loci * n_cols, 0ull);
    std::vector<uint32_t> nh((size_t)n_loci * n_cols, 0u), col(n_cols), cnt(n_cols), rec(n_loci, 0u);
    QueryKmers q;
    for (uint64_t i = 0; i < n_seqs; i++) {
        if (locus_of[i] == BIGSI_TYPING_NONE) continue;
        uint32_t nk, nu, mk;
        Hits found{nullptr, col.data(), cnt.data(), n_cols};
        search_reference_shaped(ix, seqs + offsets[i], offsets[i + 1] - offsets[i], k, threshold < 0.0 ? 0.0 : threshold, q, &nk, &nu, &mk, found);
        if (!nu) continue;
        rec[locus_of[i]]++;
        const size_t row = (size_t)locus_of[i] * n_cols;
        for (uint64_t j = 0; j < found.total; j++) {
            if (!selected(col[j])) continue;
            const uint64_t key = ((uint64_t)cnt[j] * 0xFFFFFFFFull / nu) << 32 | (uint64_t)(0xFFFFFFFFu - allele_of[i]);
            if (key > top[row + col[j]]) top[row + col[j]] = key;
            nh[row + col[j]]++;
        }
    }
    TRY(bdb_read_failed(ix));
    std::vector<uint32_t> lc((size_t)n_loci * 3, 0u), sc((size_t)n_cols * 2, 0u);
    for (uint32_t l = 0; l < n_loci; l++)
        for (uint64_t c = 0; c < n_cols; c++) {
            const uint64_t b = top[(size_t)l * n_cols + c];
            const bool exact = (b >> 32) == 0xFFFFFFFFull;
            lc[(size_t)l * 3] += b ? 1u : 0u;
            lc[(size_t)l * 3 + 1] += exact ? 1u : 0u;
            lc[(size_t)l * 3 + 2] += nh[(size_t)l * n_cols + c] > 1u ? 1u : 0u;
            sc[c * 2] += b ? 1u : 0u;
            sc[c * 2 + 1] += exact ? 1u : 0u;
        }
    if (best) memcpy(best, top.data(), top.size() * 8);
    if (hits) memcpy(hits, nh.data(), nh.size() * 4);
    memcpy(locus_counts, lc.data(), lc.size() * 4);
    memcpy(sample_counts, sc.data(), sc.size() * 4);
    memcpy(records, rec.data(), rec.size() * 4);
    return BIGSI_OK;
}

int bigsi_cpu_score_presence(int, const uint8_t *bits, const uint64_t *bit_offsets, const uint32_t *num_kmers, const uint32_t *found,
                             const uint32_t *unique, uint64_t n, bigsi_hip_hit_score *scores)
{
    if (n == 0) return BIGSI_OK;
    if (!bits || !bit_offsets || !num_kmers || !scores) return fail(BIGSI_ERR_INVALID, "NULL argument");
    static_assert(sizeof(bigsi_hip_hit_score) == sizeof(bigsi_score::HitScore), "score record layout");
    for (uint64_t t = 0; t < n; t++) {
        if (bit_offsets[t] & 7u) return fail(BIGSI_ERR_INVALID, "bit_offsets[%llu] is not a multiple of 8", (unsigned long long)t);
        const uint8_t *p = bits + bit_offsets[t];
        bigsi_score::score_hit([p](uint32_t kk) { uint64_t w; memcpy(&w, p + 8ull * kk, 8); return bigsi_score::lsb_first(w); }, num_kmers[t],
                               found ? found[t] : 0u, unique ? unique[t] : 0u, reinterpret_cast<bigsi_score::HitScore *>(&scores[t]));
    }
    return BIGSI_OK;
}

// BIGSI.search(..., score=True) for any number of sequences (the twin of bigsi_hip_search_stream_scored): the hit lists of
// bigsi_cpu_search_stream, then per sequence with hits its presence bits (graph/bigsi.py:232-237, one test per k-mer position,
// colour and hash) and Scorer.score's record (bigsi_score.hpp, the code the device compiles).
int bigsi_cpu_search_stream_scored(bigsi_cpu_index *ix, const char *seqs, const uint64_t *offsets, uint64_t n_seqs, uint32_t k,
                                   double threshold, uint32_t flags, uint32_t *num_kmers, uint32_t *num_unique, uint32_t *min_kmers,
                                   uint64_t *hit_offsets, uint32_t *colours, uint32_t *counts, uint64_t hit_capacity, uint8_t *bits,
                                   uint64_t bits_capacity, uint64_t *bit_offsets, bigsi_hip_hit_score *scores, uint64_t *bits_needed)
{
    if (!bit_offsets) return fail(BIGSI_ERR_INVALID, "bit_offsets is NULL");
    if (hit_capacity && (!colours || !scores)) return fail(BIGSI_ERR_INVALID, "colours / scores is NULL");
    bit_offsets[0] = 0;
    if (bits_needed) *bits_needed = 0;
    std::vector<uint32_t> nk_own, nu_own;
    if (!num_kmers) { nk_own.resize(n_seqs); num_kmers = nk_own.data(); }
    if (!num_unique) { nu_own.resize(n_seqs); num_unique = nu_own.data(); }
    const int rc = bigsi_cpu_search_stream(ix, seqs, offsets, n_seqs, k, threshold, flags, num_kmers, num_unique, min_kmers, hit_offsets, colours,
                                           counts, hit_capacity);
    if (rc != BIGSI_OK && rc != BIGSI_ERR_CAPACITY) return rc;
    uint64_t need = 0;
    for (uint64_t i = 0; i < n_seqs; i++) need += (hit_offsets[i + 1] - hit_offsets[i]) * (((uint64_t)num_kmers[i] + 63) / 64 * 8);
    if (bits_needed) *bits_needed = need;
    if (rc == BIGSI_ERR_CAPACITY) return rc;
    const bool fits = need <= bits_capacity && (bits || need == 0);
    std::vector<uint8_t> text;
    uint64_t at = 0;
    for (uint64_t i = 0; i < n_seqs; i++) {
        const uint64_t lo = hit_offsets[i], hi = hit_offsets[i + 1], n = num_kmers[i], bytes = (n + 63) / 64 * 8;
        if (hi == lo) continue;
        if (fits && n) {
            text.resize((hi - lo) * n);
            TRY(bigsi_cpu_presence(ix, seqs + offsets[i], offsets[i + 1] - offsets[i], k, colours + lo, (uint32_t)(hi - lo), text.data()));
        }
        for (uint64_t t = lo; t < hi; t++) {
            bit_offsets[t] = at;
            if (fits) {
                memset(&scores[t], 0, sizeof scores[t]);
                if (n) {
                    uint8_t *p = bits + at;
                    memset(p, 0, bytes);
                    const uint8_t *s = text.data() + (t - lo) * n;
                    for (uint64_t j = 0; j < n; j++)
                        if (s[j] == '1') p[j >> 3] |= (uint8_t)(0x80u >> (j & 7));
                    bigsi_score::score_hit([p](uint32_t kk) { uint64_t w; memcpy(&w, p + 8ull * kk, 8); return bigsi_score::lsb_first(w); }, (uint32_t)n,
                                           counts ? counts[t] : num_unique[i], num_unique[i], reinterpret_cast<bigsi_score::HitScore *>(&scores[t]));
                }
            }
            at += bytes;
        }
    }
    bit_offsets[hit_offsets[n_seqs]] = at;
    if (!fits) return fail(BIGSI_ERR_CAPACITY, "bit buffer holds %llu bytes, %llu needed", (unsigned long long)bits_capacity, (unsigned long long)need);
    return BIGSI_OK;
}

}  // extern "C"

// ---------------------------------------------------------------------------------------------- the exact k-mer counter
// (include/bigsi_cpu_kmercount.h.)  Plainly: every window read base by base, the canonical key taken by comparing the two packed
// words, a std::map from key to count; the filter is bigsi_cpu_bloom over the kept keys' strings, hashed as they are.

struct bigsi_cpu_kmer_counter {
    uint32_t k = 0;
    std::map<uint64_t, uint32_t> counts;
    uint64_t counted = 0, skipped = 0;
};

namespace {
inline int base_code(char ch)
{
    switch (ch) {
    case 'A': case 'a': return 0;
    case 'C': case 'c': return 1;
    case 'G': case 'g': return 2;
    case 'T': case 't': return 3;
    default: return -1;
    }
}
}  // namespace

extern "C" {

int bigsi_cpu_kmer_counter_create(int, uint32_t k, uint64_t, bigsi_cpu_kmer_counter **out)
{
    if (!out) return fail(BIGSI_ERR_INVALID, "NULL argument");
    *out = nullptr;
    if (k == 0 || k > BIGSI_KMERCOUNT_MAX_K) return fail(BIGSI_ERR_INVALID, "k must be in [1, %u], got %u", BIGSI_KMERCOUNT_MAX_K, k);
    bigsi_cpu_kmer_counter *c = new (std::nothrow) bigsi_cpu_kmer_counter();
    if (!c) return fail(BIGSI_ERR_NOMEM, "host allocation failed");
    c->k = k;
    *out = c;
    return BIGSI_OK;
}

int bigsi_cpu_kmer_counter_destroy(bigsi_cpu_kmer_counter *c)
{
    delete c;
    return BIGSI_OK;
}

int bigsi_cpu_kmer_counter_reset(bigsi_cpu_kmer_counter *c)
{
    if (!c) return fail(BIGSI_ERR_INVALID, "NULL counter");
    c->counts.clear();
    c->counted = c->skipped = 0;
    return BIGSI_OK;
}

int bigsi_cpu_kmer_counter_add(bigsi_cpu_kmer_counter *c, const char *seqs, const uint64_t *offsets, uint64_t n_seqs)
{
    if (!c) return fail(BIGSI_ERR_INVALID, "NULL counter");
    if (n_seqs == 0) return BIGSI_OK;
    if (!offsets) return fail(BIGSI_ERR_INVALID, "NULL argument");
    const uint32_t k = c->k;
    uint64_t positions = 0;
    for (uint64_t i = 0; i < n_seqs; i++) {
        if (offsets[i + 1] < offsets[i]) return fail(BIGSI_ERR_INVALID, "offsets must be non-decreasing");
        const uint64_t len = offsets[i + 1] - offsets[i];
        positions += len >= k ? len - k + 1 : 0;
    }
    if (offsets[n_seqs] - offsets[0] && !seqs) return fail(BIGSI_ERR_INVALID, "seqs is NULL");
    if (positions > 0xFFFFFFFFull - (c->counted + c->skipped))
        return fail(BIGSI_ERR_RANGE, "%llu more positions behind %llu: a k-mer counter takes at most 2^32 - 1 in its lifetime",
                    (unsigned long long)positions, (unsigned long long)(c->counted + c->skipped));
    for (uint64_t i = 0; i < n_seqs; i++) {
        const char *s = seqs + offsets[i];
        const uint64_t len = offsets[i + 1] - offsets[i];
        for (uint64_t p = 0; p + k <= len; p++) {
            uint64_t fwd = 0, rc = 0;
            bool ok = true;
            for (uint32_t j = 0; j < k && ok; j++) {
                const int f = base_code(s[p + j]), r = base_code(s[p + k - 1 - j]);
                ok = f >= 0 && r >= 0;
                fwd = (fwd << 2) | (uint64_t)(f & 3);
                rc = (rc << 2) | (uint64_t)(3 - (r & 3));
            }
            if (!ok) { c->skipped++; continue; }
            c->counted++;
            c->counts[std::min(fwd, rc)]++;
        }
    }
    return BIGSI_OK;
}

int bigsi_cpu_kmer_counter_info(bigsi_cpu_kmer_counter *c, uint64_t out[4])
{
    if (!c || !out) return fail(BIGSI_ERR_INVALID, "NULL argument");
    out[0] = c->counted;
    out[1] = c->skipped;
    out[2] = c->counts.size();
    out[3] = 0;
    return BIGSI_OK;
}

int bigsi_cpu_kmer_counter_spectrum(bigsi_cpu_kmer_counter *c, uint64_t out[256])
{
    if (!c || !out) return fail(BIGSI_ERR_INVALID, "NULL argument");
    memset(out, 0, 256 * sizeof(uint64_t));
    for (const auto &kv : c->counts) out[std::min<uint32_t>(kv.second, 255)]++;
    return BIGSI_OK;
}

int bigsi_cpu_kmer_counter_fetch(bigsi_cpu_kmer_counter *c, uint64_t *keys, uint32_t *counts, uint64_t capacity, uint64_t *n)
{
    if (!c || !n) return fail(BIGSI_ERR_INVALID, "NULL argument");
    *n = c->counts.size();
    if (capacity < *n) return fail(BIGSI_ERR_CAPACITY, "the table holds %llu k-mers, the buffers %llu", (unsigned long long)*n, (unsigned long long)capacity);
    if (*n == 0) return BIGSI_OK;
    if (!keys || !counts) return fail(BIGSI_ERR_INVALID, "NULL argument");
    uint64_t i = 0;
    for (const auto &kv : c->counts) { keys[i] = kv.first; counts[i] = kv.second; i++; }
    return BIGSI_OK;
}

int bigsi_cpu_kmer_counter_bloom(bigsi_cpu_kmer_counter *c, uint64_t m, uint32_t h, uint32_t min_count, uint8_t *out)
{
    if (!c || !out) return fail(BIGSI_ERR_INVALID, "NULL argument");
    if (m == 0 || h == 0) return fail(BIGSI_ERR_INVALID, "m and h must be > 0");
    if (min_count == 0) return fail(BIGSI_ERR_INVALID, "min_count must be >= 1");
    const uint32_t k = c->k;
    std::string kept;
    for (const auto &kv : c->counts) {
        if (kv.second < min_count) continue;
        for (uint32_t j = 0; j < k; j++) kept.push_back("ACGT"[(kv.first >> (2 * (k - 1 - j))) & 3]);
    }
    return bigsi_cpu_bloom(0, kept.data(), kept.size() / k, k, m, h, BIGSI_BLOOM_RAW, out);
}

}  // extern "C"
