// bigsi_rowsfile.hpp -- what the file <-> HBM pipeline (bigsi_rows_pipeline, bigsi_hip.hip) does on the file's side: plain host
// C++, no HIP (bigsi_rowsfile.cpp; tests/c_host/rowsfile_host.cpp drives it without a device).
#pragma once
#include "bigsi_bdb.hpp"      // BigsiBdb: BerkeleyDB hash files without libdb (shared with libbigsi_cpu.so)
#include "bigsi_hip.h"

int bigsi_fail(int code, const char *fmt, ...) __attribute__((format(printf, 2, 3)));      // (bigsi_hip.hip: sets bigsi_hip_last_error)

// pread / pwrite of [off, off + len) with up to `threads` host threads, one per 4 MiB at the most; 0 or errno
int bigsi_file_io(int fd, bool write, uint8_t *buf, uint64_t off, uint64_t len, unsigned threads);
unsigned bigsi_io_threads();                       // the host threads of a file <-> HBM call that names none: min(16, max(1, hw / 4))
unsigned bigsi_scan_threads(unsigned threads);     // ... of a BerkeleyDB page scan: independent 4 MB reads, it takes more of them
constexpr uint64_t kBigsiIoChunkBytes = 256ull << 20;      // one pinned buffer of the file <-> HBM pipeline
constexpr uint64_t kStripeParts = 16, kStripeBytes = 4ull << 20;
// The file side of load_rows_file / save_rows_file (single index and group).  `path` is a FILE (rows back to back from file_offset
// on) or, when it ends in '/', a DIRECTORY holding the same rows striped RAID-0 fashion over kParts part files: writes to one
// file are serialised by its inode lock and its page-cache tree -- 16 threads put 3.6-5.3 GB/s into ONE fresh tmpfs file
// (pwrite or mmap alike) and 63 GB/s into 16 files (scripts/probe/tmpfs_write_probe.py, mmap_write_probe.cpp) -- so a save that is
// to run at the PCIe rate needs several inodes.  Stripe s (rows [s * S, (s + 1) * S) of the range) lives in part s % P at
// row offset (s / P) * S; `layout` in the directory records P, S, row_bytes and the row count, and a load reads it back.
struct BigsiRowsFile {
    bool striped = false;
    bool bdb = false;                      // `path` is a BerkeleyDB hash file: rows are its "<row>:bitarray" records (loads only)
    BigsiBdb db;
    std::vector<BigsiBdb::Loc> loc;        // bdb: where row row0 + i lives
    int fd = -1;
    std::vector<int> fds;
    uint64_t parts = 0, stripe_rows = 0, row_bytes = 0, file_offset = 0;
    int open_(const char *path, bool save, uint64_t file_offset_, uint64_t row_bytes_, uint64_t n_rows, uint64_t row0 = 0, unsigned threads = 1);     // BIGSI_OK or an error (message set)
    uint64_t chunk_rows() const;                                           // rows per pinned buffer
    int io(bool write, uint8_t *buf, uint64_t rel_row, uint64_t n, unsigned threads) const;      // rows [rel_row, +n) of the range; 0 or errno
    int sync_all() const;
    void close_();
};
