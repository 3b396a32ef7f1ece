// bigsi_rowsfile.cpp -- the file side of bulk ingest and snapshots (bigsi_rowsfile.hpp): threaded pread / pwrite, the striped directory,
// BerkeleyDB stores as a source of rows.  Plain host C++: part of libbigsi_hip.so, and compiled by g++ for tests/c_host/rowsfile_host.cpp.
#include "bigsi_rowsfile.hpp"

#include <fcntl.h>

#include <algorithm>
#include <mutex>

#include "bigsi_launch.hpp"      // round_up, ceil_div

#define fail bigsi_fail

unsigned bigsi_io_threads() { return std::min(16u, std::max(1u, std::thread::hardware_concurrency() / 4)); }
// (the scan is independent 4 MB reads + a few hundred bytes of parsing per page: it takes more threads than the file <-> HBM pipeline)
unsigned bigsi_scan_threads(unsigned threads) { return std::max(threads, std::min(48u, std::max(1u, std::thread::hardware_concurrency() / 4))); }

// read / write [off, off + len) of the file into / from buf with up to `threads` threads; returns 0 or errno
int bigsi_file_io(int fd, bool write, uint8_t *buf, uint64_t off, uint64_t len, unsigned threads)
{
    threads = std::max(1u, std::min<unsigned>(threads, (unsigned)ceil_div(std::max<uint64_t>(len, 1), 4ull << 20)));
    std::atomic<int> err{0};
    auto work = [&](uint64_t a, uint64_t b) {
        while (a < b && !err.load()) {
            const ssize_t r = write ? pwrite(fd, buf + (a - off), (size_t)std::min<uint64_t>(b - a, 1ull << 30), (off_t)a)
                                    : pread(fd, buf + (a - off), (size_t)std::min<uint64_t>(b - a, 1ull << 30), (off_t)a);
            if (r < 0) { if (errno == EINTR) continue; err.store(errno); return; }
            if (r == 0) { err.store(write ? EIO : ENODATA); return; }      // short file
            a += (uint64_t)r;
        }
    };
    if (threads == 1) { work(off, off + len); return err.load(); }
    std::vector<std::thread> pool;
    const uint64_t per = round_up(ceil_div(len, threads), 1ull << 20);
    for (unsigned t = 0; t < threads; t++) {
        const uint64_t a = off + std::min<uint64_t>((uint64_t)t * per, len), b = off + std::min<uint64_t>((uint64_t)(t + 1) * per, len);
        if (a < b) pool.emplace_back(work, a, b);
    }
    for (auto &th : pool) th.join();
    return err.load();
}
// ---- BerkeleyDB hash files: csrc/bigsi_bdb.hpp (shared with the CPU twin)

// bigsi_hip_bdb_small_records meets every row record on its way; an import calls bigsi_hip_load_rows_file on the same file next,
// which would scan it again: the row locations of the LAST file scanned are kept (one entry, identified by device / inode / size /
// mtime) and handed to the loader, which consumes them.
struct BdbScanCache {
    std::mutex mu;
    bool valid = false;
    dev_t dev = 0; ino_t ino = 0; off_t size = 0; struct timespec mtime {};
    std::vector<std::pair<uint64_t, BigsiBdb::Loc>> rows;      // (row id, where)
};
static BdbScanCache g_bdb_cache;

// The records of a BerkeleyDB hash file that are NOT rows -- the index integers and the sample metadata, a few bytes each --
// packed as [u32 key_len][u32 value_len][key][value]...; "<row>:bitarray" records are counted and measured only.
extern "C" int bigsi_hip_bdb_small_records(const char *path, uint8_t *out, uint64_t capacity, uint64_t *needed, uint64_t *n_rows, uint64_t *max_row_bytes,
                                           uint32_t threads)
{
    if (!path || !needed) return fail(BIGSI_ERR_INVALID, "NULL argument");
    if (threads == 0) threads = bigsi_io_threads();
    const int fd = open(path, O_RDONLY);
    if (fd < 0) return fail(BIGSI_ERR_INVALID, "%s: %s", path, strerror(errno));
    BigsiBdb db;
    int rc = db.open_fd(fd) ? fail(BIGSI_ERR_INVALID, "%s: %s", path, db.error.c_str()) : BIGSI_OK;
    struct Small { std::string key; BigsiBdb::Loc loc; };
    std::vector<Small> small;
    std::mutex mu;
    std::atomic<uint64_t> rows{0}, widest{0};
    threads = bigsi_scan_threads(threads);
    std::vector<std::vector<std::pair<uint64_t, BigsiBdb::Loc>>> found(threads);      // row locations, per scanning thread
    if (rc == BIGSI_OK && db.scan(threads, [&](unsigned tid, const uint8_t *key, uint32_t klen, const BigsiBdb::Loc &l) {
            uint64_t r;
            if (bigsi_bdb_row_key(key, klen, &r)) {
                rows++;
                uint64_t w = widest.load();
                while (l.len > w && !widest.compare_exchange_weak(w, l.len)) {}
                found[tid].emplace_back(r, l);
                return;
            }
            std::lock_guard<std::mutex> g(mu);
            small.push_back(Small{std::string(reinterpret_cast<const char *>(key), klen), l});
        }))
        rc = fail(BIGSI_ERR_INVALID, "%s: %s", path, db.error.c_str());
    if (rc == BIGSI_OK) {
        struct stat sb;
        std::lock_guard<std::mutex> g(g_bdb_cache.mu);
        g_bdb_cache.valid = false;
        g_bdb_cache.rows.clear();
        if (fstat(fd, &sb) == 0) {
            for (auto &v : found) { g_bdb_cache.rows.insert(g_bdb_cache.rows.end(), v.begin(), v.end()); std::vector<std::pair<uint64_t, BigsiBdb::Loc>>().swap(v); }
            g_bdb_cache.dev = sb.st_dev; g_bdb_cache.ino = sb.st_ino; g_bdb_cache.size = sb.st_size; g_bdb_cache.mtime = sb.st_mtim;
            g_bdb_cache.valid = true;
        }
    }
    uint64_t need = 0;
    if (rc == BIGSI_OK) {
        std::sort(small.begin(), small.end(), [](const Small &a, const Small &b) { return a.key < b.key; });      // (threads meet the pages in any order)
        for (auto &s_ : small) need += 8 + s_.key.size() + s_.loc.len;
        *needed = need;
        if (n_rows) *n_rows = rows.load();
        if (max_row_bytes) *max_row_bytes = widest.load();
        if (out && capacity < need) rc = fail(BIGSI_ERR_CAPACITY, "buffer holds %llu bytes, %llu needed", (unsigned long long)capacity, (unsigned long long)need);
        else if (out) {
            std::vector<uint8_t> page;
            uint8_t *q = out;
            for (auto &s_ : small) {
                const uint32_t kl = (uint32_t)s_.key.size(), vl = s_.loc.len;
                memcpy(q, &kl, 4); memcpy(q + 4, &vl, 4); memcpy(q + 8, s_.key.data(), kl);
                const int e = db.read_value(s_.loc, q + 8 + kl, vl, page);
                if (e) { rc = fail(BIGSI_ERR_INVALID, "%s: reading the value of %s: %s", path, s_.key.c_str(), e == EILSEQ ? "corrupt overflow chain" : strerror(e)); break; }
                q += 8 + kl + vl;
            }
        }
    }
    close(fd);
    return rc;
}

// ---- BigsiRowsFile (bigsi_rowsfile.hpp): one file, or a directory of striped part files
int BigsiRowsFile::open_(const char *path, bool save, uint64_t file_offset_, uint64_t row_bytes_, uint64_t n_rows, uint64_t row0, unsigned threads)
{
    file_offset = file_offset_;
    row_bytes = row_bytes_;
    const size_t len = strlen(path);
    striped = len > 0 && path[len - 1] == '/';
    if (!striped) {
        fd = open(path, save ? (O_WRONLY | O_CREAT) : O_RDONLY, 0644);
        if (fd < 0) return fail(BIGSI_ERR_INVALID, "%s: %s", path, strerror(errno));
        if (!save && file_offset == 0 && BigsiBdb::is_bdb(fd)) {
            // a v0.3 BerkeleyDB store: one scan of its hash pages locates the "<row>:bitarray" records of the range; io() then
            // gathers rows from wherever they are (inline, or an overflow chain of pages)
            bdb = true;
            int rc = db.open_fd(fd) ? fail(BIGSI_ERR_INVALID, "%s", db.error.c_str()) : BIGSI_OK;
            if (rc == BIGSI_OK) {
                loc.assign(n_rows, BigsiBdb::Loc{});
                bool cached = false;
                {
                    // the scan bigsi_hip_bdb_small_records has just made of this very file (same inode, size and mtime), if any
                    struct stat sb;
                    std::lock_guard<std::mutex> g(g_bdb_cache.mu);
                    if (g_bdb_cache.valid && fstat(fd, &sb) == 0 && sb.st_dev == g_bdb_cache.dev && sb.st_ino == g_bdb_cache.ino && sb.st_size == g_bdb_cache.size &&
                        sb.st_mtim.tv_sec == g_bdb_cache.mtime.tv_sec && sb.st_mtim.tv_nsec == g_bdb_cache.mtime.tv_nsec) {
                        for (auto &e : g_bdb_cache.rows)
                            if (e.first >= row0 && e.first - row0 < n_rows) loc[e.first - row0] = e.second;
                        cached = true;
                        if (row0 == 0 && n_rows >= g_bdb_cache.rows.size()) { g_bdb_cache.valid = false; std::vector<std::pair<uint64_t, BigsiBdb::Loc>>().swap(g_bdb_cache.rows); }      // consumed
                    }
                }
                if (!cached && db.scan(bigsi_scan_threads(threads), [&](unsigned, const uint8_t *key, uint32_t klen, const BigsiBdb::Loc &l) {
                        uint64_t r;
                        if (bigsi_bdb_row_key(key, klen, &r) && r >= row0 && r - row0 < n_rows) loc[r - row0] = l;      // (one writer per row: a key occurs once)
                    }))
                    rc = fail(BIGSI_ERR_INVALID, "%s", db.error.c_str());
            }
            if (rc != BIGSI_OK) { char keep[512]; snprintf(keep, sizeof keep, "%s", bigsi_hip_last_error()); close_(); return fail(rc, "%s: %s", path, keep); }
        }
        return BIGSI_OK;
    }
    const std::string dir(path);
    const std::string lay = dir + "layout";
    if (save) {
        if (mkdir(dir.substr(0, len - 1).c_str(), 0755) != 0 && errno != EEXIST) return fail(BIGSI_ERR_INVALID, "mkdir %s: %s", path, strerror(errno));
        parts = kStripeParts;
        stripe_rows = std::max<uint64_t>(1, kStripeBytes / row_bytes);
        FILE *f = fopen(lay.c_str(), "w");
        if (!f) return fail(BIGSI_ERR_INVALID, "%s: %s", lay.c_str(), strerror(errno));
        fprintf(f, "bigsi-rows-striped 1\nparts %llu\nstripe_rows %llu\nrow_bytes %llu\nrows %llu\nfile_offset %llu\n", (unsigned long long)parts,
                (unsigned long long)stripe_rows, (unsigned long long)row_bytes, (unsigned long long)n_rows, (unsigned long long)file_offset);
        fclose(f);
    } else {
        FILE *f = fopen(lay.c_str(), "r");
        if (!f) return fail(BIGSI_ERR_INVALID, "%s: %s", lay.c_str(), strerror(errno));
        unsigned long long ver = 0, p_ = 0, s_ = 0, rb_ = 0, rows_ = 0, fo_ = 0;
        const int got = fscanf(f, "bigsi-rows-striped %llu parts %llu stripe_rows %llu row_bytes %llu rows %llu file_offset %llu", &ver, &p_, &s_, &rb_, &rows_, &fo_);
        fclose(f);
        if (got != 6 || ver != 1 || p_ == 0 || p_ > 4096 || s_ == 0) return fail(BIGSI_ERR_INVALID, "%s is not a striped rows layout", lay.c_str());
        if (rb_ != row_bytes || fo_ != file_offset || rows_ < n_rows)
            return fail(BIGSI_ERR_INVALID, "%s holds %llu rows of %llu bytes (offset %llu); asked for %llu rows of %llu bytes (offset %llu)", lay.c_str(), rows_, rb_, fo_,
                        (unsigned long long)n_rows, (unsigned long long)row_bytes, (unsigned long long)file_offset);
        parts = p_;
        stripe_rows = s_;
    }
    for (uint64_t p = 0; p < parts; p++) {
        char name[32];
        snprintf(name, sizeof name, "part.%03llu", (unsigned long long)p);
        // (a part file of an earlier, longer save must not keep its tail: the parts of a save that starts at offset 0 are cut to size)
        const int f = open((dir + name).c_str(), save ? (O_WRONLY | O_CREAT | (file_offset == 0 ? O_TRUNC : 0)) : O_RDONLY, 0644);
        if (f < 0) { const int e = errno; close_(); return fail(BIGSI_ERR_INVALID, "%s%s: %s", path, name, strerror(e)); }
        fds.push_back(f);
    }
    return BIGSI_OK;
}

uint64_t BigsiRowsFile::chunk_rows() const
{
    uint64_t per = std::max<uint64_t>(1, kBigsiIoChunkBytes / row_bytes);
    if (striped && per > stripe_rows * parts) per -= per % (stripe_rows * parts);      // whole rounds over the parts: every part file gets the same share of a chunk
    return per;
}

int BigsiRowsFile::io(bool write, uint8_t *buf, uint64_t rel_row, uint64_t n, unsigned threads) const
{
    if (bdb) {
        if (write) return EROFS;
        // rows of the store, zero-extended (or cut) to row_bytes; a row the store does not hold reads as zeros
        const unsigned T = (unsigned)std::max<uint64_t>(1, std::min<uint64_t>(threads, ceil_div(n, 64)));
        std::atomic<int> err{0};
        std::atomic<uint64_t> next{0};
        auto work = [&]() {
            std::vector<uint8_t> page;
            for (;;) {
                const uint64_t a = next.fetch_add(64);
                if (a >= n || err.load()) return;
                for (uint64_t i = a; i < std::min(n, a + 64); i++) {
                    const BigsiBdb::Loc &l = loc[rel_row + i];
                    uint8_t *dst = buf + i * row_bytes;
                    const uint32_t take = l.kind ? (uint32_t)std::min<uint64_t>(l.len, row_bytes) : 0u;
                    if (take) { const int e = db.read_value(l, dst, take, page); if (e) { err.store(e); return; } }
                    if (take < row_bytes) memset(dst + take, 0, row_bytes - take);
                }
            }
        };
        if (T == 1) work();
        else {
            std::vector<std::thread> pool;
            for (unsigned t = 0; t < T; t++) pool.emplace_back(work);
            for (auto &th : pool) th.join();
        }
        return err.load();
    }
    if (!striped) return bigsi_file_io(fd, write, buf, file_offset + rel_row * row_bytes, n * row_bytes, threads);
    // a thread owns the part files p == t (mod T): no two threads inside one inode
    const unsigned T = (unsigned)std::max<uint64_t>(1, std::min<uint64_t>(std::min<uint64_t>(threads, parts), ceil_div(n, stripe_rows)));
    std::atomic<int> err{0};
    auto work = [&](unsigned t) {
        const uint64_t s0 = rel_row / stripe_rows, s1 = ceil_div(rel_row + n, stripe_rows);
        for (uint64_t s = s0; s < s1 && !err.load(); s++) {
            const uint64_t p = s % parts;
            if (p % T != t) continue;
            const uint64_t a = std::max(rel_row, s * stripe_rows), b = std::min(rel_row + n, (s + 1) * stripe_rows);
            uint64_t off = file_offset + ((s / parts) * stripe_rows + (a - s * stripe_rows)) * row_bytes, left = (b - a) * row_bytes;
            uint8_t *q = buf + (a - rel_row) * row_bytes;
            while (left && !err.load()) {
                const ssize_t r = write ? pwrite(fds[p], q, (size_t)left, (off_t)off) : pread(fds[p], q, (size_t)left, (off_t)off);
                if (r < 0) { if (errno == EINTR) continue; err.store(errno); break; }
                if (r == 0) { err.store(write ? EIO : ENODATA); break; }
                q += r; off += (uint64_t)r; left -= (uint64_t)r;
            }
        }
    };
    if (T == 1) { work(0); return err.load(); }
    std::vector<std::thread> pool;
    for (unsigned t = 0; t < T; t++) pool.emplace_back(work, t);
    for (auto &th : pool) th.join();
    return err.load();
}

int BigsiRowsFile::sync_all() const
{
    int e = 0;
    if (fd >= 0 && fsync(fd) != 0 && errno != EINVAL && errno != EROFS) e = errno;
    for (int f : fds)
        if (fsync(f) != 0 && errno != EINVAL && errno != EROFS) e = errno;
    return e;
}

void BigsiRowsFile::close_()
{
    if (fd >= 0) close(fd);
    for (int f : fds) close(f);
    fd = -1;
    fds.clear();
}
