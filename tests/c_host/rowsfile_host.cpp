// A stand-alone program (its own main) over the file side of bulk ingest and snapshots (bigsi_amd/csrc/bigsi_rowsfile.cpp: plain
// host C++, no device): bigsi_file_io, BigsiRowsFile on a flat file, on a striped directory and on a BerkeleyDB store, the scan
// cache between bigsi_hip_bdb_small_records and BigsiRowsFile::open_.  Files are checked against a naive model written here: one
// pwrite / pread per row, part index and offset computed the slow way.  tests/test_rows_file_host.py compiles it with g++ together
// with bigsi_rowsfile.cpp, once with -fsanitize=address,undefined and once with -fsanitize=thread, and runs both.
//
//     rowsfile_host files <empty directory>                                   flat file and striped directory; prints "rows file host: ok"
//     rowsfile_host bdb <store> <row0> <n> <row_bytes> <threads> <route> <out> [<other store>]
//         route plain:     the rows [row0, +n) of the store, gathered through open_ / io, written to <out>.rows
//         route cached:    the same after bigsi_hip_bdb_small_records has scanned the store (its records go to <out>.small)
//         route rewritten: the scan, then <store> is overwritten in place with <other store>'s bytes (a later mtime), then the rows
// Test infrastructure only: nothing in the product loads this file.
#include <fcntl.h>
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <sys/stat.h>
#include <unistd.h>

#include <string>
#include <vector>

#include "../../bigsi_amd/csrc/bigsi_rowsfile.hpp"

static char g_msg[1024] = "";
int bigsi_fail(int code, const char *fmt, ...)      // the library's is in bigsi_hip.hip: this one records the message all the same
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_msg, sizeof g_msg, fmt, ap);
    va_end(ap);
    return code;
}
extern "C" const char *bigsi_hip_last_error(void) { return g_msg; }

#define CHECK(cond, ...)                                  \
    do {                                                  \
        if (!(cond)) {                                    \
            fprintf(stderr, "FAILED %s:%d %s: ", __FILE__, __LINE__, #cond); \
            fprintf(stderr, __VA_ARGS__);                 \
            fprintf(stderr, " [last error: %s]\n", g_msg); \
            exit(1);                                      \
        }                                                 \
    } while (0)

static std::vector<uint8_t> random_bytes(uint64_t n, uint64_t seed)
{
    std::vector<uint8_t> v((n + 7) / 8 * 8);
    uint64_t s = seed * 0x9E3779B97F4A7C15ull + 1;
    for (uint64_t i = 0; i < v.size(); i += 8) {
        s ^= s << 13; s ^= s >> 7; s ^= s << 17;
        memcpy(v.data() + i, &s, 8);
    }
    v.resize(n);
    return v;
}

static std::vector<uint8_t> slurp(const std::string &path)
{
    FILE *f = fopen(path.c_str(), "rb");
    CHECK(f, "%s: %s", path.c_str(), strerror(errno));
    std::vector<uint8_t> v;
    std::vector<uint8_t> buf(1 << 20);
    for (size_t got; (got = fread(buf.data(), 1, buf.size(), f)) > 0;) v.insert(v.end(), buf.begin(), buf.begin() + got);
    fclose(f);
    return v;
}

static void dump(const std::string &path, const uint8_t *p, uint64_t n)
{
    FILE *f = fopen(path.c_str(), "wb");
    CHECK(f && fwrite(p, 1, n, f) == n && fclose(f) == 0, "%s: %s", path.c_str(), strerror(errno));
}

static std::string part_name(const std::string &dir, const char *stem, uint64_t p)
{
    char name[64];
    snprintf(name, sizeof name, "%s.%03llu", stem, (unsigned long long)p);
    return dir + name;
}

// the model: row r of the range goes to its place with one pwrite of its own
static void model_flat(const std::string &path, const uint8_t *rows, uint64_t n, uint64_t rb, uint64_t file_offset)
{
    const int fd = open(path.c_str(), O_WRONLY | O_CREAT | O_TRUNC, 0644);
    CHECK(fd >= 0, "%s", path.c_str());
    for (uint64_t r = 0; r < n; r++) CHECK(pwrite(fd, rows + r * rb, rb, (off_t)(file_offset + r * rb)) == (ssize_t)rb, "row %llu", (unsigned long long)r);
    close(fd);
}

static void model_striped(const std::string &dir, const uint8_t *rows, uint64_t n, uint64_t rb, uint64_t parts, uint64_t stripe_rows)
{
    for (uint64_t p = 0; p < parts; p++) close(open(part_name(dir, "model", p).c_str(), O_WRONLY | O_CREAT | O_TRUNC, 0644));
    for (uint64_t r = 0; r < n; r++) {
        uint64_t stripe = 0, in_stripe = r;
        while (in_stripe >= stripe_rows) { in_stripe -= stripe_rows; stripe++; }      // stripe = r / S, slowly
        uint64_t part = stripe, round = 0;
        while (part >= parts) { part -= parts; round++; }                             // part = stripe % P, round = stripe / P
        const int fd = open(part_name(dir, "model", part).c_str(), O_WRONLY);
        CHECK(fd >= 0 && pwrite(fd, rows + r * rb, rb, (off_t)((round * stripe_rows + in_stripe) * rb)) == (ssize_t)rb, "row %llu", (unsigned long long)r);
        close(fd);
    }
}

static void expect_rows(const BigsiRowsFile &rf, const uint8_t *rows, uint64_t rel, uint64_t n, unsigned threads, std::vector<uint8_t> &buf)
{
    buf.assign(n * rf.row_bytes + 1, 0xAB);
    const int e = rf.io(false, buf.data(), rel, n, threads);
    CHECK(e == 0, "io(read, %llu, +%llu, %u threads): %s", (unsigned long long)rel, (unsigned long long)n, threads, strerror(e));
    CHECK(memcmp(buf.data(), rows + rel * rf.row_bytes, n * rf.row_bytes) == 0 && buf.back() == 0xAB, "rows [%llu, +%llu) with %u threads differ",
          (unsigned long long)rel, (unsigned long long)n, threads);
}

// ---------------------------------------------------------------------------------------------- (a) one flat file
static void flat_case(const std::string &dir, uint64_t rb, uint64_t file_offset, uint64_t n, uint64_t cut, unsigned t0, unsigned t1)
{
    const std::string path = dir + "flat.bin", model = dir + "flat.model";
    const std::vector<uint8_t> rows = random_bytes(n * rb, rb);
    std::vector<uint8_t> buf;
    unlink(path.c_str());
    {
        BigsiRowsFile rf;
        CHECK(rf.open_(path.c_str(), true, file_offset, rb, n) == BIGSI_OK && !rf.striped && !rf.bdb, "open for save");
        CHECK(rf.chunk_rows() == kBigsiIoChunkBytes / rb, "chunk_rows");
        CHECK(rf.io(true, const_cast<uint8_t *>(rows.data()), 0, cut, t0) == 0, "first range");                      // two uneven ranges
        CHECK(rf.io(true, const_cast<uint8_t *>(rows.data()) + cut * rb, cut, n - cut, t1) == 0, "second range");
        CHECK(rf.sync_all() == 0, "fsync");
        rf.close_();
    }
    model_flat(model, rows.data(), n, rb, file_offset);
    const std::vector<uint8_t> got = slurp(path);
    CHECK(got.size() == file_offset + n * rb && got == slurp(model), "the file is not the model's (size %llu)", (unsigned long long)got.size());
    {
        BigsiRowsFile rf;
        CHECK(rf.open_(path.c_str(), false, file_offset, rb, n) == BIGSI_OK && !rf.bdb, "open for load");
        expect_rows(rf, rows.data(), 0, n, t1, buf);
        expect_rows(rf, rows.data(), cut / 3, n / 2, t0, buf);
        expect_rows(rf, rows.data(), n - 1, 1, 5, buf);
        rf.close_();
    }
    CHECK(truncate(path.c_str(), (off_t)(file_offset + (n - 1) * rb)) == 0, "truncate");                              // one row short
    {
        BigsiRowsFile rf;
        CHECK(rf.open_(path.c_str(), false, file_offset, rb, n) == BIGSI_OK, "open the short file");
        buf.assign(n * rb, 0);
        for (unsigned t : {1u, t1}) CHECK(rf.io(false, buf.data(), 0, n, t) == ENODATA, "a short file reads as ENODATA (%u threads)", t);
        expect_rows(rf, rows.data(), 0, n - 1, t1, buf);
        rf.close_();
    }
    BigsiRowsFile none;
    CHECK(none.open_((dir + "nothing.bin").c_str(), false, file_offset, rb, n) == BIGSI_ERR_INVALID && strstr(g_msg, "nothing.bin"), "a missing file");
    unlink(path.c_str());
    unlink(model.c_str());
}

// ---------------------------------------------------------------------------------------------- (b) a striped directory
static void striped_case(const std::string &top)
{
    const uint64_t rb = (512u << 10) + 24, P = kStripeParts, S = kStripeBytes / rb, n = P * S * 2 + 5;      // every part twice, the end inside a stripe
    CHECK(S >= 2 && S < 64, "stripe_rows %llu", (unsigned long long)S);
    const std::string dir = top + "striped/";
    const std::vector<uint8_t> rows = random_bytes(n * rb, 7);
    std::vector<uint8_t> buf;
    char want_layout[256];
    auto save = [&](uint64_t n_rows, uint64_t cut, unsigned t0, unsigned t1) {
        BigsiRowsFile rf;
        CHECK(rf.open_(dir.c_str(), true, 0, rb, n_rows) == BIGSI_OK && rf.striped && rf.parts == P && rf.stripe_rows == S, "open for save");
        CHECK(rf.io(true, const_cast<uint8_t *>(rows.data()), 0, cut, t0) == 0, "first range");
        CHECK(rf.io(true, const_cast<uint8_t *>(rows.data()) + cut * rb, cut, n_rows - cut, t1) == 0, "second range");
        CHECK(rf.sync_all() == 0, "fsync");
        rf.close_();
        model_striped(dir, rows.data(), n_rows, rb, P, S);
        uint64_t total = 0;
        for (uint64_t p = 0; p < P; p++) {
            const std::vector<uint8_t> got = slurp(part_name(dir, "part", p));
            CHECK(got == slurp(part_name(dir, "model", p)), "part %llu of %llu rows is not the model's (size %llu)", (unsigned long long)p,
                  (unsigned long long)n_rows, (unsigned long long)got.size());
            total += got.size();
        }
        CHECK(total == n_rows * rb, "part sizes");
        snprintf(want_layout, sizeof want_layout, "bigsi-rows-striped 1\nparts %llu\nstripe_rows %llu\nrow_bytes %llu\nrows %llu\nfile_offset 0\n",
                 (unsigned long long)P, (unsigned long long)S, (unsigned long long)rb, (unsigned long long)n_rows);
        const std::vector<uint8_t> lay = slurp(dir + "layout");
        CHECK(std::string(lay.begin(), lay.end()) == want_layout, "layout text");
    };
    save(n, 3 * S + 2, 5, (unsigned)P + 4);                              // both ranges start or end inside a stripe
    {
        BigsiRowsFile rf;
        CHECK(rf.open_(dir.c_str(), false, 0, rb, n) == BIGSI_OK && rf.striped && rf.parts == P && rf.stripe_rows == S, "open for load");
        const uint64_t per = rf.chunk_rows();
        CHECK(per > 0 && per % (P * S) == 0 && per <= kBigsiIoChunkBytes / rb && per + P * S > kBigsiIoChunkBytes / rb, "chunk_rows %llu", (unsigned long long)per);
        expect_rows(rf, rows.data(), 0, n, (unsigned)P, buf);
        expect_rows(rf, rows.data(), 3, n - 20, 1, buf);
        expect_rows(rf, rows.data(), S + 2, P * S + 3, 5, buf);
        expect_rows(rf, rows.data(), 2 * S - 1, n - 2 * S, (unsigned)P + 24, buf);
        expect_rows(rf, rows.data(), P * S + 1, 1, 3, buf);
        rf.close_();
        BigsiRowsFile fewer;                                             // fewer rows than the layout records: fine
        CHECK(fewer.open_(dir.c_str(), false, 0, rb, n - 9) == BIGSI_OK, "a load of fewer rows");
        expect_rows(fewer, rows.data(), 1, n - 10, 5, buf);
        fewer.close_();
    }
    const uint64_t n2 = 4 * S + 2;                                       // a shorter save at offset 0 over the same directory: the parts are cut
    save(n2, S - 1, 4, 1);
    for (uint64_t p = 0; p < P; p++) {
        struct stat sb;
        CHECK(stat(part_name(dir, "part", p).c_str(), &sb) == 0 && (uint64_t)sb.st_size == (p < 4 ? S : p == 4 ? 2 : 0) * rb, "part %llu after the shorter save", (unsigned long long)p);
    }
    struct Bad { uint64_t rb, off, n; };
    for (const Bad &b : {Bad{rb + 8, 0, n2}, Bad{rb, 8, n2}, Bad{rb, 0, n2 + 1}}) {
        BigsiRowsFile rf;
        CHECK(rf.open_(dir.c_str(), false, b.off, b.rb, b.n) == BIGSI_ERR_INVALID && strstr(g_msg, "holds"), "a load the layout does not cover");
        rf.close_();
    }
    CHECK(unlink((dir + "layout").c_str()) == 0, "unlink layout");
    BigsiRowsFile rf;
    CHECK(rf.open_(dir.c_str(), false, 0, rb, n2) == BIGSI_ERR_INVALID && strstr(g_msg, "layout"), "a directory without layout");
    rf.close_();
    for (uint64_t p = 0; p < P; p++) {
        unlink(part_name(dir, "part", p).c_str());
        unlink(part_name(dir, "model", p).c_str());
    }
    rmdir(dir.substr(0, dir.size() - 1).c_str());
}

// ---------------------------------------------------------------------------------------------- (c) rows of a BerkeleyDB store
static void small_records(const char *store, unsigned threads, const std::string &out)
{
    uint64_t need = 0, n_rows = 0, widest = 0;
    CHECK(bigsi_hip_bdb_small_records(store, nullptr, 0, &need, &n_rows, &widest, threads) == BIGSI_OK, "the scan");
    std::vector<uint8_t> blob(need + 1, 0xAB);
    uint64_t need2 = 0;
    if (need) CHECK(bigsi_hip_bdb_small_records(store, blob.data(), need - 1, &need2, nullptr, nullptr, threads) == BIGSI_ERR_CAPACITY, "a buffer too small");
    CHECK(bigsi_hip_bdb_small_records(store, blob.data(), need, &need2, &n_rows, &widest, threads) == BIGSI_OK && need2 == need && blob[need] == 0xAB, "the records");
    dump(out + ".small", blob.data(), need);
    printf("rows %llu widest %llu\n", (unsigned long long)n_rows, (unsigned long long)widest);
}

static int bdb_case(int argc, char **argv)
{
    CHECK(argc >= 9, "usage");
    const char *store = argv[2];
    const uint64_t row0 = strtoull(argv[3], nullptr, 10), n = strtoull(argv[4], nullptr, 10), rb = strtoull(argv[5], nullptr, 10);
    const unsigned threads = (unsigned)strtoul(argv[6], nullptr, 10);
    const std::string route = argv[7], out = argv[8];
    if (route != "plain") small_records(store, threads, out);
    if (route == "rewritten") {
        CHECK(argc >= 10, "usage");
        struct stat before;
        CHECK(stat(store, &before) == 0, "stat");
        const std::vector<uint8_t> other = slurp(argv[9]);
        const int fd = open(store, O_WRONLY | O_TRUNC);                  // the same inode, other contents
        CHECK(fd >= 0 && write(fd, other.data(), other.size()) == (ssize_t)other.size(), "rewrite");
        const struct timespec ts[2] = {before.st_atim, {before.st_mtim.tv_sec + 1, before.st_mtim.tv_nsec}};
        CHECK(futimens(fd, ts) == 0 && close(fd) == 0, "futimens");
    }
    BigsiRowsFile rf;
    CHECK(rf.open_(store, false, 0, rb, n, row0, threads) == BIGSI_OK && rf.bdb && !rf.striped, "open the store");
    std::vector<uint8_t> buf(n * rb + 1, 0xAB);
    const uint64_t cut = n / 3 + 1;
    CHECK(rf.io(false, buf.data(), 0, cut, threads) == 0 && rf.io(false, buf.data() + cut * rb, cut, n - cut, threads) == 0 && buf.back() == 0xAB, "gather");
    CHECK(rf.io(true, buf.data(), 0, 1, threads) == EROFS, "a store is read-only");
    rf.close_();
    dump(out + ".rows", buf.data(), n * rb);
    return 0;
}

int main(int argc, char **argv)
{
    if (argc >= 2 && strcmp(argv[1], "bdb") == 0) return bdb_case(argc, argv);
    CHECK(argc == 3 && strcmp(argv[1], "files") == 0, "usage: rowsfile_host files <dir> | bdb ...");
    const std::string top = std::string(argv[2]) + "/";
    CHECK(bigsi_io_threads() >= 1 && bigsi_io_threads() <= 16 && bigsi_scan_threads(3) >= 3 && bigsi_scan_threads(100) == 100, "thread rules");
    // bigsi_file_io itself: 12 MiB + 1 at offset 5, with more threads than its one-per-4-MiB cap allows
    {
        const std::vector<uint8_t> bytes = random_bytes((12u << 20) + 1, 3);
        std::vector<uint8_t> back(bytes.size() + 1, 0xAB);
        const std::string path = top + "plain.bin";
        const int fd = open(path.c_str(), O_RDWR | O_CREAT | O_TRUNC, 0644);
        CHECK(fd >= 0 && bigsi_file_io(fd, true, const_cast<uint8_t *>(bytes.data()), 5, bytes.size(), 9) == 0, "threaded write");
        CHECK(bigsi_file_io(fd, false, back.data(), 5, bytes.size(), 2) == 0 && memcmp(back.data(), bytes.data(), bytes.size()) == 0 && back.back() == 0xAB, "read back");
        CHECK(bigsi_file_io(fd, false, back.data(), 6, bytes.size(), 4) == ENODATA && bigsi_file_io(fd, false, back.data(), 0, 0, 4) == 0, "beyond the end; nothing");
        close(fd);
        unlink(path.c_str());
    }
    flat_case(top, 125, 4096, 1000, 377, 1, 3);
    flat_case(top, 12504, 4096, 800, 123, 3, 3);          // 10 MB: bigsi_file_io really splits it over three threads
    striped_case(top);
    printf("rows file host: ok\n");
    return 0;
}
