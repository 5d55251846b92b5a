// host_ingest.cpp -- FASTA reader, check_sequence and the 2-bit slot packer (host side; no GPU): the mapping cache, the record
// tables of the two readers, the one-pass reader's copies and the C entry points.  Bytes -> slots is fasta_pack.h, the reader's
// threads are ingest_threads.h.
//
// Restates, as one pass over the file bytes, what the reference does with Python line iteration:
//   idelucs/utils.py:137-188 / :224-260  record state machine ('#' skipped, '>' flushes the current
//                                        record only if an id is set, id = line[1:-1], other lines
//                                        .strip()ped and joined, unconditional flush at EOF)
//   idelucs/utils.py:26-51               check_sequence (header checks, translate, delete, validate)
// and produces the packed slot layout documented in include/idelucs_hip.h.
#include <fcntl.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>
#include <sys/mman.h>
#include <sys/stat.h>
#include <unistd.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "common.h"
#include "dev_env.h"
#include "fasta_pack.h"
#include "ingest_threads.h"

// ------------------------------------------------------------------------------------------------
// FASTA reader.  The reference walks the file line by line in Python (utils.py:137-188, :224-260); here
// the file is read once, header lines are located by a parallel newline scan, the record table is built
// by the reference's state machine applied to the header lines only, and records are validated / counted
// and later translated + packed by a pool of threads straight from the raw bytes (no cleaned copy
// unless the caller asks for one).  Semantics kept exactly, including the quirks: sequence lines seen
// before a record id is set (file start, or after an empty-id header) roll into the next flushed record
// (`lines` is only reset on a flush, utils.py:184/257); the first failing record in file order decides
// the error.
// ------------------------------------------------------------------------------------------------
namespace {

struct Rec {
    size_t id_b, id_e;       // id bytes in buf (line[1:-1])
    size_t data_b, data_e;   // file range whose non-'#', non-'>' lines are this record's sequence
    int64_t len;             // cleaned length
};

// chr(b) as UTF-8 (the reference formats chr(stripped[0]) into the message, utils.py:47-49)
std::string chr_utf8(uint8_t b)
{
    std::string s;
    if (b < 0x80) s.push_back((char)b);
    else { s.push_back((char)(0xC0 | (b >> 6))); s.push_back((char)(0x80 | (b & 0x3F))); }
    return s;
}

double now_ms() { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

// utils.py:37-40 header checks.  (A record without id bytes passes: that is also the empty file's one record, whose buf is NULL
// and must not reach memchr.)
int header_kind(const uint8_t *buf, const Rec &r)
{
    if (r.id_e <= r.id_b) return REC_OK;
    const uint8_t h0 = buf[r.id_b];
    if (h0 == '>' || h0 == '#' || py_bytes_space(h0) || (h0 >= 0x1c && h0 <= 0x1f)) return REC_BAD_HEADER;
    if (memchr(buf + r.id_b, '\t', r.id_e - r.id_b)) return REC_TAB;
    return REC_OK;
}

// the reference's message for a record that failed with `kind` (byte: the invalid one of REC_BAD_BASE); returns the error code
int report_bad_record(const uint8_t *buf, const Rec &r, int kind, uint8_t byte)
{
    if (kind == REC_BAD_HEADER) { idl::set_error("Bad character in sequence header"); return IDL_ERR_HEADER; }
    if (kind == REC_TAB) { idl::set_error("tab included in header"); return IDL_ERR_HEADER; }
    const std::string id((const char *)buf + r.id_b, r.id_e - r.id_b);
    idl::set_error("Invalid DNA byte in sequence %s: '%s'", id.c_str(), chr_utf8(byte).c_str());
    return IDL_ERR_BASE;
}

int g_last_bind_node = -1;      // what the last job was bound to (idl_ingest_numa_node)
int g_last_file_node = -1;      // ... and where it found the file's pages (-1: not asked, not resident, spread, or not permitted)

}  // namespace

struct FileMap {                  // read-only view of the whole file (mmap; empty files map to nothing)
    const uint8_t *p = nullptr;
    size_t n = 0;
    bool unmap_inline = false;    // (idl_ingest_release: the caller wants the unmapping finished when the call returns)
    // munmap of a large mapping walks every page (25 ms for a 1 GB file, measured) and holds the process's memory-map lock while
    // it does: by default it runs on a detached thread
    ~FileMap()
    {
        if (!p || !n) return;
        void *q = (void *)p;
        const size_t len = n;
        if (unmap_inline || len < ((size_t)64 << 20)) { munmap(q, len); return; }
        try { std::thread([q, len]() { munmap(q, len); }).detach(); } catch (...) { munmap(q, len); }
    }
};

// A mapped file is shared by the handles that read it and KEPT after the last one closes, until another file is opened or
// idl_ingest_release() is called: a run reads its input more than once (the feature store, then the un-mutated vectors of every
// predict: reference models.py:147-163 re-reads the file per voter), and unmapping a 1 GB file costs 25 ms of the memory-map lock,
// during which everything else the process allocates waits -- it landed either on the feature buffer's allocation or on the
// first launches of the epoch, wherever the close was put.
struct MapKey { dev_t dev = 0; ino_t ino = 0; off_t size = -1; long msec = 0, mnsec = 0;
                bool operator==(const MapKey &o) const { return dev == o.dev && ino == o.ino && size == o.size && msec == o.msec && mnsec == o.mnsec; } };
std::mutex g_map_mu;
MapKey g_map_key;
std::shared_ptr<FileMap> g_map;

struct MapRef {
    std::shared_ptr<FileMap> m;
    const uint8_t *data() const { return m ? m->p : nullptr; }
    size_t size() const { return m ? m->n : 0; }
};

// maps fd (size > 0) or returns the kept mapping of the same file (device, inode, size, modification time); false: mmap failed
bool acquire_map(int fd, const struct stat &st, MapRef *out)
{
    const MapKey key{st.st_dev, st.st_ino, st.st_size, (long)st.st_mtim.tv_sec, (long)st.st_mtim.tv_nsec};
    std::lock_guard<std::mutex> lk(g_map_mu);
    if (g_map && g_map_key == key) { out->m = g_map; return true; }
    void *m = mmap(nullptr, (size_t)st.st_size, PROT_READ, MAP_PRIVATE, fd, 0);
    if (m == MAP_FAILED) return false;
    (void)madvise(m, (size_t)st.st_size, MADV_SEQUENTIAL);
    auto fm = std::make_shared<FileMap>();
    fm->p = (const uint8_t *)m;
    fm->n = (size_t)st.st_size;
    g_map = fm;                    // (the mapping kept before goes when its last handle does)
    g_map_key = key;
    out->m = fm;
    return true;
}

// opens a regular file and sizes it: the descriptor, or -1 (cannot open) / -2 (cannot size, not a regular file)
static int open_regular(const char *path, struct stat *st)
{
    const int fd = open(path, O_RDONLY);
    if (fd < 0) return -1;
    if (fstat(fd, st) != 0 || !S_ISREG(st->st_mode)) { close(fd); return -2; }
    return fd;
}

// the mapping of the file at `path` for a reader; an empty file maps to nothing (*empty says so: the general reader reads it as
// one empty record, the one-pass reader declines it).  IDL_ERR_IO with the message set when it cannot be opened, sized or mapped.
static int map_file(const char *path, MapRef *out, bool *empty)
{
    struct stat st;
    const int fd = open_regular(path, &st);
    if (fd < 0) { idl::set_error(fd == -1 ? "cannot open %s" : "cannot size %s", path); return IDL_ERR_IO; }
    *empty = st.st_size == 0;
    const bool mapped = *empty || acquire_map(fd, st, out);
    close(fd);
    if (!mapped) { idl::set_error("cannot map %s", path); return IDL_ERR_IO; }
    return IDL_OK;
}

struct idl_fasta {
    MapRef buf;
    std::vector<Rec> recs;
    int check = 1;
    int64_t total_bases = 0, total_slots = 0, names_bytes = 0;
    int names_high = -1;           // 1: some header byte is >= 0x80 (the decoded-name checks apply), 0: all ASCII, -1: this reader did not look
    std::vector<int64_t> arena_slot;      // idl_fasta_parse_pack: first slot of every record in the caller's arenas (+ the end)
    std::vector<int64_t> lengths;         // idl_fasta_parse_pack: cleaned lengths, ready for idl_fasta_arena_meta
    std::vector<uint8_t> mask_sent;       // idl_fasta_parse_pack with device arenas: 1 = the record's invalid-mask was copied there
    int64_t n_mask_unsent = 0;
    int64_t min_len = 0, max_len = 0;
};

namespace {

// One record of an opened handle: its cleaned bytes to bdst and / or its packed slots to cdst / mdst (either may be NULL).
void pack_record(const uint8_t *buf, const Rec &r, int check, uint8_t *bdst, uint8_t *cdst, uint8_t *mdst)
{
    const uint8_t *p = buf + r.data_b, *e = buf + r.data_e;
    uint8_t bb = 0;
    if (!cdst) {
        if (check) { CopySink s{{}, bdst}; (void)clean_range(p, e, s, &bb); }
        else raw_range(p, e, [&](uint8_t c) { *bdst++ = c; });
        return;
    }
    const Packer at{(uint32_t *)cdst, (uint32_t *)mdst};
    const int64_t slots = (r.len + 63) / 64;
    // INVALID BYTES: the non-CHECKED sinks skip them.  The file was validated when it was opened, but the mapping is MAP_PRIVATE
    // of a file that somebody may rewrite underneath it: packing an opened handle never fails, and with r.len fixed at the open
    // it stays inside the record's (len + 63) / 64 slots as long as the bytes are what they were.  (The one-pass reader, which
    // sees the bytes for the first time, reports them: one_pass_slice.)
    if (check && bdst) { PackCopySink s{at, bdst}; (void)clean_range(p, e, s, &bb); s.pk.finish(slots); }
    else if (check) { PackOnlySink s{at}; (void)clean_range(p, e, s, &bb); s.pk.finish(slots); }
    else {
        Packer pk = at;
        if (bdst) raw_range(p, e, [&](uint8_t c) { *bdst++ = c; pk.push(T.code[c]); });
        else raw_range(p, e, [&](uint8_t c) { pk.push(T.code[c]); });
        pk.finish(slots);
    }
}

// Records [lo, lo + m) of a handle on nt threads, each a run of records of about equal cleaned bases: record lo + i goes to
// bytes + boff[i] (cleaned bytes; bytes may be NULL) and to codes + soff[i] * 16 / mask + soff[i] * 8 (codes may be NULL).
// boff is the prefix sum of the m cleaned lengths (m + 1 entries, from 0).
void pack_records(const idl_fasta *f, int64_t lo, int64_t m, const int64_t *boff, const int64_t *soff, int nt, uint8_t *bytes,
                  uint8_t *codes, uint8_t *mask)
{
    const uint8_t *buf = f->buf.data();
    const int64_t total = boff[m];
    parallel_for(nt, [&](int t) {
        // balance by cleaned bases
        const int64_t b_lo = total * t / nt, b_hi = total * (t + 1) / nt;
        int64_t i0 = std::lower_bound(boff, boff + m, b_lo) - boff;
        const int64_t i1 = (t == nt - 1) ? m : std::lower_bound(boff, boff + m, b_hi) - boff;
        if (t == 0) i0 = 0;
        for (int64_t i = i0; i < i1; ++i)
            pack_record(buf, f->recs[(size_t)(lo + i)], f->check, bytes ? bytes + boff[i] : nullptr, codes ? codes + soff[i] * 16 : nullptr,
                        codes ? mask + soff[i] * 8 : nullptr);
    });
}

}  // namespace

extern "C" {

int idl_check_sequence(const uint8_t *in, int64_t len, uint8_t *out, int64_t *out_len, int64_t *bad_pos)
{
    IDL_REQUIRE(len >= 0 && (len == 0 || (in && out)) && out_len, "NULL buffer");
    int64_t n = 0;
    for (int64_t i = 0; i < len; ++i) {
        const uint8_t t = T.translate[in[i]];
        if (t == 0) continue;
        if (t == 1) {
            if (bad_pos) *bad_pos = i;
            idl::set_error("Invalid DNA byte: '%s'", chr_utf8(in[i]).c_str());
            return IDL_ERR_BASE;
        }
        out[n++] = t;
    }
    *out_len = n;
    return IDL_OK;
}

int idl_pack(const uint8_t *bytes, const int64_t *byte_off, int64_t n, uint8_t *codes, uint8_t *mask,
             int64_t *slot_off)
{
    IDL_REQUIRE(n >= 0 && byte_off && slot_off, "NULL buffer");
    int64_t slot = 0;
    for (int64_t s = 0; s < n; ++s) {
        const int64_t len = byte_off[s + 1] - byte_off[s];
        IDL_REQUIRE(len >= 0, "byte_off not ascending");
        slot_off[s] = slot;
        slot += (len + 63) / 64;
    }
    slot_off[n] = slot;
    if (slot > 0) IDL_REQUIRE(bytes && codes && mask, "NULL buffer");
    const int nt = (n >= 64) ? n_threads() : 1;
    parallel_for(nt, [&](int t) {
        for (int64_t s = n * t / nt; s < n * (t + 1) / nt; ++s) {
            const int64_t len = byte_off[s + 1] - byte_off[s];
            if (len <= 0) continue;
            Packer pk{(uint32_t *)(codes + slot_off[s] * 16), (uint32_t *)(mask + slot_off[s] * 8)};
            for (const uint8_t *b = bytes + byte_off[s], *e = b + len; b < e; ++b) pk.push(T.code[*b]);
            pk.finish((len + 63) / 64);
        }
    });
    return IDL_OK;
}

int idl_fasta_open(const char *path, int check, idl_fasta **out)
{
    IDL_REQUIRE(path && out, "NULL argument");
    *out = nullptr;
    std::unique_ptr<idl_fasta> f(new idl_fasta());
    f->check = check;
    bool empty = false;
    if (const int rc = map_file(path, &f->buf, &empty)) return rc;
    const uint8_t *buf = f->buf.data();
    const size_t size = f->buf.size();
    const int nt = (size > par_min_bytes() && size >= 64) ? n_threads() : 1;
    const bool timing = getenv("IDELUCS_INGEST_TIMING") != nullptr;
    const double t_0 = now_ms();

    // 1. header lines ('>' at a line start), found by a parallel newline scan.  (This first touch of the mapping also takes its page
    // faults -- about 4 of the 10 ms at 1 GB; madvise(MADV_POPULATE_READ) per slice was 3 x slower, measured.)
    std::vector<std::vector<size_t>> hdr((size_t)nt);
    parallel_for(nt, [&](int t) {
        const size_t b = size * (size_t)t / (size_t)nt, e = size * (size_t)(t + 1) / (size_t)nt;
        size_t p = b;
        if (b == 0) { if (size > 0 && buf[0] == '>') hdr[t].push_back(0); }
        while (p < e) {
            const uint8_t *nl = (const uint8_t *)memchr(buf + p, '\n', e - p);
            if (!nl) break;
            p = (size_t)(nl - buf) + 1;
            if (p < size && buf[p] == '>') hdr[t].push_back(p);
        }
    });

    const double t_1 = now_ms();
    // 2. the reference's state machine over the header lines
    size_t cur_b = 0;
    bool have_id = false;
    size_t id_b = 0, id_e = 0;
    auto line_end = [&](size_t hs) -> size_t {
        const uint8_t *nl = (const uint8_t *)memchr(buf + hs, '\n', size - hs);
        return nl ? (size_t)(nl - buf) + 1 : size;
    };
    for (int t = 0; t < nt; ++t) {
        for (size_t hs : hdr[t]) {
            const size_t he = line_end(hs);
            if (have_id && id_e > id_b) {            // seq_id != "": flush, `lines` restart after this header
                f->recs.push_back(Rec{id_b, id_e, cur_b, hs, 0});
                cur_b = he;
            }
            // id = line[1:-1]: drops exactly one trailing byte whatever it is
            id_b = hs + 1;
            id_e = (he - hs >= 2) ? he - 1 : id_b;
            if (id_e < id_b) id_e = id_b;
            have_id = true;
        }
    }
    f->recs.push_back(Rec{have_id ? id_b : 0, have_id ? id_e : 0, cur_b, size, 0});   // unconditional flush at EOF

    const double t_2 = now_ms();
    // 3. validate + count, in parallel; the first failing record in file order decides the error
    const int64_t n = (int64_t)f->recs.size();
    const int nt2 = (size > par_min_bytes() && n >= 2) ? n_threads() : 1;
    std::vector<int64_t> first_bad((size_t)nt2, -1);
    std::vector<int> bad_kind((size_t)nt2, REC_OK);
    std::vector<uint8_t> bad_byte((size_t)nt2, 0);
    // balance by bytes: thread t takes the records whose data starts in its slice of the file
    std::vector<int64_t> cut((size_t)nt2 + 1, n);
    cut[0] = 0;
    {
        int t = 1;
        for (int64_t i = 0; i < n && t < nt2; ++i)
            while (t < nt2 && f->recs[(size_t)i].data_b >= size * (size_t)t / (size_t)nt2) cut[(size_t)t++] = i;
    }
    parallel_for(nt2, [&](int t) {
        for (int64_t i = cut[(size_t)t]; i < cut[(size_t)t + 1]; ++i) {
            Rec &r = f->recs[(size_t)i];
            uint8_t bb = 0;
            int kind = check ? header_kind(buf, r) : REC_OK;
            if (kind == REC_OK) {
                CountSink s{};
                if (check) kind = clean_range(buf + r.data_b, buf + r.data_e, s, &bb);
                else raw_range(buf + r.data_b, buf + r.data_e, [&](uint8_t) { ++s.cnt; });
                r.len = s.cnt;
            }
            if (kind != REC_OK) { first_bad[(size_t)t] = i; bad_kind[(size_t)t] = kind; bad_byte[(size_t)t] = bb; break; }
        }
    });
    for (int t = 0; t < nt2; ++t)
        if (first_bad[(size_t)t] >= 0) return report_bad_record(buf, f->recs[(size_t)first_bad[(size_t)t]], bad_kind[(size_t)t], bad_byte[(size_t)t]);
    if (timing) fprintf(stderr, "idl_fasta_open: header scan %.1f ms, record table %.1f ms, validate + count %.1f ms (%d threads)\n", t_1 - t_0, t_2 - t_1, now_ms() - t_2, nt);
    for (const Rec &r : f->recs) {
        f->total_bases += r.len;
        f->total_slots += (r.len + 63) / 64;
        f->names_bytes += (int64_t)(r.id_e - r.id_b);
    }
    *out = f.release();
    return IDL_OK;
}

}  // extern "C"

// ------------------------------------------------------------------------------------------------
// One pass over the file: locate, validate, count and 2-bit pack at the same time (idl_fasta_open + idl_fasta_pack_range read
// the bytes three times: header scan, validate + count, pack).  Thread t owns the records whose header line starts in its slice
// of the file and packs them back to back into ITS region of the caller's arenas, so no thread needs another's lengths; the
// vectoriser takes every record's first slot from slot_off[] and its slot count from its length, so the gaps between the regions
// are never read.  With device arenas of the same shape, each thread also sends what it has packed (hipMemcpyAsync from the
// pinned arena, every few MB) while it goes on parsing.
// The reference's rolling semantics (sequence lines seen before an id is set belong to the NEXT flushed record: data before the
// first header, headers with an empty id) are left to the general reader: IDL_FALLBACK, as for check == 0 files, for a region
// that runs out of slots (records of a few bases each) -- the caller then uses idl_fasta_open.
// ------------------------------------------------------------------------------------------------
namespace {

// this library's own copy streams (+ the events that tie them to the caller's stream), per device, made on first use and kept
struct CopyStreams {
    std::vector<hipStream_t> extra;
    std::vector<hipEvent_t> done;
    hipEvent_t start = nullptr;
};

CopyStreams *copy_streams(int dev, int count)
{
    static std::mutex mu;
    static std::vector<std::pair<int, CopyStreams *>> all;
    std::lock_guard<std::mutex> lk(mu);
    for (auto &p : all) if (p.first == dev && (int)p.second->extra.size() == count) return p.second;
    CopyStreams *c = new CopyStreams();
    bool ok = hipEventCreateWithFlags(&c->start, hipEventDisableTiming) == hipSuccess;
    for (int i = 0; ok && i < count; ++i) {
        hipStream_t s = nullptr;
        hipEvent_t e = nullptr;
        ok = hipStreamCreateWithFlags(&s, hipStreamNonBlocking) == hipSuccess && hipEventCreateWithFlags(&e, hipEventDisableTiming) == hipSuccess;
        if (ok) { c->extra.push_back(s); c->done.push_back(e); }
    }
    if (!ok) { delete c; return nullptr; }       // (leaks what was made; the caller goes on with its one stream)
    all.emplace_back(dev, c);
    return c;
}

struct FastOut {
    std::vector<Rec> recs;
    std::vector<int64_t> slot;
    std::vector<uint8_t> mask_sent;                 // per record: 1 = its invalid-mask went to the device with its piece (0: the caller rebuilds it from the length)
    double t_begin = 0, t_end = 0, t_send = 0;      // IDELUCS_INGEST_TIMING: when this thread started / finished, host time inside its copy calls
    int n_send = 0;
    int fallback = 0, bad_kind = REC_OK, copy_failed = 0;
    uint8_t bad_byte = 0;
    Rec bad_rec{};
};

// what the slices of one idl_fasta_parse_pack call share
struct OnePass {
    const uint8_t *buf;
    size_t size;
    uint8_t *codes, *mask;                  // the caller's host arenas, cap_slots slots
    int64_t cap_slots;
    void *dev_codes, *dev_mask;             // device arenas of the same shape, or NULL
    std::vector<hipStream_t> streams;       // thread t copies on stream t mod count
    CopyStreams *cs = nullptr;              // where streams[1 ..] come from
    int per_thread, ns;                     // slices per thread, slices
    int64_t region_slots;                   // a slice's expected slots
    int copy_div;
    std::vector<int> sched;                 // the piece schedule: cuts in % of region_slots
    int64_t COPY_SLOTS, COPY_MIN;           // a piece's largest / (but for the last) smallest size
    bool sparse_mask, timing;
    std::vector<FastOut> outs;              // per slice
};

// the pieces of one slice's region on their way to the device
struct PieceSender {
    const OnePass &j;
    FastOut &o;
    hipStream_t stream;
    int64_t sent;                           // slots [region_lo, sent) have been sent
    bool piece_dirty = false;               // a record since the last copy holds an N
    void send(int64_t upto)
    {
        // the invalid-mask is a third of the bytes, and on clean input it says nothing the lengths do not: a piece without an N
        // sends its packed bases only, and its records are flagged for the caller to rebuild their masks on the device
        const bool with_mask = piece_dirty || !j.sparse_mask;
        if (j.dev_codes != nullptr && upto > sent) {
            const double ts = j.timing ? now_ms() : 0.0;
            if (hipMemcpyAsync((uint8_t *)j.dev_codes + sent * 16, j.codes + sent * 16, (size_t)(upto - sent) * 16, hipMemcpyHostToDevice, stream) != hipSuccess ||
                (with_mask && hipMemcpyAsync((uint8_t *)j.dev_mask + sent * 8, j.mask + sent * 8, (size_t)(upto - sent) * 8, hipMemcpyHostToDevice, stream) != hipSuccess))
                o.copy_failed = 1;
            if (j.timing) { o.t_send += now_ms() - ts; o.n_send += with_mask ? 2 : 1; }
        }
        o.mask_sent.resize(o.recs.size(), (j.dev_codes != nullptr && with_mask) ? 1 : 0);
        piece_dirty = false;
        sent = upto;
    }
};

enum { REC_REGION_FULL = -1 };              // (beside REC_*: the slice's region of the arenas has no room for the line)

// slice sl of the file, on thread t: the records whose header line starts in it, into its region of the arenas
void one_pass_slice(OnePass &j, const int t, const int sl)
{
    const uint8_t *buf = j.buf;
    const size_t size = j.size;
    const int ns = j.ns;
    FastOut &o = j.outs[(size_t)sl];
    if (j.timing) o.t_begin = now_ms();
    const size_t b = size * (size_t)sl / (size_t)ns, e = size * (size_t)(sl + 1) / (size_t)ns;
    const int64_t region_lo = j.cap_slots * sl / ns, region_hi = j.cap_slots * (sl + 1) / ns;
    auto line_end = [&](size_t p) -> size_t {
        const uint8_t *nl = find_nl(buf + p, size - p);
        return nl ? (size_t)(nl - buf) + 1 : size;
    };
    size_t q = b;
    if (b > 0) q = line_end(b - 1);                               // the first line that STARTS in this slice
    // the first header line at or after q (thread 0 also vouches for everything before the file's first header: '#' lines only)
    while (q < size && buf[q] != '>') {
        if (sl == 0) { if (buf[q] != '#') { o.fallback = 1; return; } }
        else if (q >= e) return;                                  // no record starts in this slice
        q = line_end(q);
    }
    if (q >= size) { if (sl == 0) o.fallback = 1; return; }       // (slice 0: a file without any header line)
    if (q >= e) return;
    int64_t slot = region_lo;
    size_t cut = 0;                                               // next entry of the piece schedule
    const bool one_cut = j.per_thread > 1 && ns > 1;              // several slices per thread: one cut per slice, at 70 %
    PieceSender snd{j, o, j.streams[(size_t)t % j.streams.size()], region_lo};
    size_t hs = q;
    while (hs < size && hs < e) {                                 // one record per turn; it may run past e
        const size_t he = line_end(hs);
        Rec r{hs + 1, (he - hs >= 2) ? he - 1 : hs + 1, he, he, 0};   // id = line[1:-1]: drops exactly one trailing byte whatever it is
        if (r.id_e <= r.id_b) { o.fallback = 1; return; }         // empty id: the general reader's rolling semantics
        uint8_t bb = 0;
        int kind = header_kind(buf, r);
        // INVALID BYTES: this reader sees the bytes for the first time, so its sink is the CHECKED one: it reports them
        PackCheckedSink sink{Packer{(uint32_t *)(j.codes + slot * 16), (uint32_t *)(j.mask + slot * 8)}};
        const uint8_t *lp = buf + he;
        if (kind == REC_OK)                                       // the record's lines: up to the next '>' line
            kind = visit_seq_lines(lp, buf + size, PrefetchNl(), [](uint8_t c) { return c == '>'; }, [&](const uint8_t *a, const uint8_t *bnd) {
                if (slot + (sink.cnt + (int64_t)(bnd - a)) / 64 + 2 > region_hi) return (int)REC_REGION_FULL;
                return clean_line(a, bnd, sink, &bb);
            });
        if (kind == REC_REGION_FULL) { o.fallback = 1; return; }
        if (kind != REC_OK) { o.bad_kind = kind; o.bad_byte = bb; o.bad_rec = r; return; }
        r.data_e = (size_t)(lp - buf);
        r.len = sink.cnt;
        const int64_t slots = (r.len + 63) / 64;
        sink.pk.finish(slots);
        snd.piece_dirty |= sink.pk.dirty;
        o.recs.push_back(r);
        o.slot.push_back(slot);
        slot += slots;
        if (slot - snd.sent >= j.COPY_SLOTS) snd.send(slot);
        else if (!j.copy_div && cut < (one_cut ? std::min<size_t>(j.sched.size(), 1) : j.sched.size()) &&
                 (slot - region_lo) * 100 >= j.region_slots * (one_cut ? 70 : j.sched[cut]) && slot - snd.sent >= j.COPY_MIN) {
            snd.send(slot);
            if (one_cut) cut = j.sched.size();
            while (cut < j.sched.size() && (slot - region_lo) * 100 >= j.region_slots * j.sched[cut]) ++cut;
        }
        hs = r.data_e;
    }
    snd.send(slot);
    o.slot.push_back(slot);                                       // end of this slice's records
    if (j.timing) o.t_end = now_ms();
}

// A thread sends what it has packed while it goes on parsing; what is still unsent when it finishes is the copy TAIL every
// later stage waits for.  Round 4 cut a region into 3 equal pieces: the last third of everything (125 MB at cfg2) left when the
// parsing was over, 2.6 ms at the link's 48 GB/s (IDELUCS_INGEST_TIMING=2: threads joined 8.0 ms, copies drained 10.6).  The
// pieces now shrink -- cuts at 45 / 75 / 92 % of the region's expected slots, the rest at the end (IDELUCS_DEV=copy_sched="45,75,92")
// -- for the same number of calls as four equal pieces: every hipMemcpyAsync takes the stream's lock and ~15 us of host time
// (8 equal pieces 14.6 ms against 12.3-12.8 for 2-4, 16 pieces 18.9: round 4).  A piece is at most 6 MB (big files: more
// pieces) and, but for the last, at least 384 KB.  IDELUCS_DEV=copy_div=<d> keeps round 4's d equal pieces for A/B runs.
void set_copy_schedule(OnePass &j)
{
    j.region_slots = (int64_t)(j.size / 64) / j.ns + 1;
    j.copy_div = idl::dev_env_int("copy_div", 0, 1, 64);
    const char *e = idl::dev_env("copy_sched");
    for (const char *p = e ? e : "45,75,92"; *p;) {       // (of a thread's share; with several slices per thread: of each slice, first cut only)
        char *q = nullptr;
        const long x = strtol(p, &q, 10);
        if (q == p) break;
        if (x > 0 && x < 100 && (j.sched.empty() || x > j.sched.back())) j.sched.push_back((int)x);
        p = (*q == ',') ? q + 1 : q;
    }
    const int64_t COPY_MAX = (int64_t)1 << 18;
    j.COPY_MIN = (int64_t)1 << 14;
    j.COPY_SLOTS = j.copy_div ? std::min<int64_t>(COPY_MAX, std::max<int64_t>(j.COPY_MIN, j.region_slots / j.copy_div)) : COPY_MAX;
}

// copy streams: the caller's, and IDELUCS_DEV=copy_streams - 1 more of this library's own (thread t copies on stream t mod count;
// they start behind whatever the caller's stream holds and the caller's stream waits for them at the end).  false: a HIP call failed.
bool open_copy_streams(OnePass &j, hipStream_t stream, int dev)
{
    j.streams.assign(1, stream);
    const int want = idl::dev_env_int("copy_streams", 1, 1, 8);
    j.cs = want > 1 ? copy_streams(dev, want - 1) : nullptr;
    if (j.cs == nullptr) return true;
    if (hipEventRecord(j.cs->start, stream) != hipSuccess) j.cs = nullptr;
    for (size_t i = 0; j.cs != nullptr && i < j.cs->extra.size(); ++i) {
        if (hipStreamWaitEvent(j.cs->extra[i], j.cs->start, 0) != hipSuccess) return false;
        j.streams.push_back(j.cs->extra[i]);
    }
    return true;
}

// the IDELUCS_INGEST_TIMING line of idl_fasta_parse_pack
void report_timeline(const OnePass &j, double t_0, const std::vector<double> &th_begin, const std::vector<double> &th_end, hipStream_t stream, int bind_node)
{
    double b_max = 0, e_min = 1e300, e_max = 0, snd = 0;
    int n_calls = 0;
    for (size_t t = 0; t < th_end.size(); ++t) {
        if (th_end[t] == 0) continue;
        b_max = std::max(b_max, th_begin[t] - t_0); e_min = std::min(e_min, th_end[t] - t_0); e_max = std::max(e_max, th_end[t] - t_0);
    }
    for (const FastOut &o : j.outs) { snd += o.t_send; n_calls += o.n_send; }
    const double t_join = now_ms() - t_0;
    double t_drain = -1;
    // IDELUCS_INGEST_TIMING=2 also waits for the copies here (diagnostic only: the caller overlaps this wait with its own work)
    if (j.dev_codes != nullptr && atoi(getenv("IDELUCS_INGEST_TIMING")) >= 2 && hipStreamSynchronize(stream) == hipSuccess) t_drain = now_ms() - t_0;
    fprintf(stderr, "idl_fasta_parse_pack timeline: last thread started %.2f ms, threads finished %.2f .. %.2f, joined %.2f, copies drained %.2f; "
                    "%d slices, %d copy calls on %zu stream(s), %.2f ms of host time in them (sum over threads); bound to node %d (the file's pages: node %d)\n",
            b_max, e_min, e_max, t_join, t_drain, j.ns, n_calls, j.streams.size(), snd, bind_node, g_last_file_node);
}

// merge: every thread copies its records to their place in the file's order (prefix of the per-thread counts) and sums its own
size_t merge_slices(idl_fasta *f, const std::vector<FastOut> &outs, int nt)
{
    const uint8_t *buf = f->buf.data();
    const int ns = (int)outs.size();
    std::vector<size_t> first((size_t)ns + 1, 0);
    for (int t = 0; t < ns; ++t) first[(size_t)t + 1] = first[(size_t)t] + outs[(size_t)t].recs.size();
    const size_t n = first[(size_t)ns];
    f->recs.resize(n);
    f->arena_slot.resize(n + 1);
    f->lengths.resize(n);
    f->mask_sent.resize(n);
    int64_t last_end = 0;
    for (const FastOut &o : outs) if (!o.recs.empty()) last_end = o.slot.back();
    f->arena_slot[n] = last_end;
    struct Part { int64_t bases = 0, slots = 0, names = 0, lo = INT64_MAX, hi = 0, unsent = 0; unsigned high = 0; };
    std::vector<Part> parts((size_t)ns);
    parallel_for(n >= 4096 ? nt : 1, [&](int t0) {
        for (int t = t0; t < ns; t += (n >= 4096 ? nt : 1)) {
            const FastOut &o = outs[(size_t)t];
            Part &p = parts[(size_t)t];
            const size_t at = first[(size_t)t];
            for (size_t i = 0; i < o.recs.size(); ++i) {
                const Rec &r = o.recs[i];
                f->recs[at + i] = r;
                f->arena_slot[at + i] = o.slot[i];
                f->lengths[at + i] = r.len;
                const uint8_t ms = i < o.mask_sent.size() ? o.mask_sent[i] : 0;
                f->mask_sent[at + i] = ms;
                p.unsent += ms ? 0 : 1;
                p.bases += r.len; p.slots += (r.len + 63) / 64; p.names += (int64_t)(r.id_e - r.id_b);
                for (size_t j = r.id_b; j < r.id_e; ++j) p.high |= buf[j];      // (a non-ASCII header: the caller validates the decoded names at once)
                p.lo = std::min(p.lo, r.len); p.hi = std::max(p.hi, r.len);
            }
        }
    });
    int64_t lo = INT64_MAX;
    unsigned high = 0;
    for (const Part &p : parts) {
        f->total_bases += p.bases; f->total_slots += p.slots; f->names_bytes += p.names; f->n_mask_unsent += p.unsent;
        high |= p.high;
        lo = std::min(lo, p.lo); f->max_len = std::max(f->max_len, p.hi);
    }
    f->min_len = n ? lo : 0;
    f->names_high = (high & 0x80u) ? 1 : 0;
    return n;
}

}  // namespace

extern "C" {

int idl_fasta_parse_pack(const char *path, uint8_t *codes, uint8_t *mask, int64_t cap_slots, void *dev_codes, void *dev_mask,
                         void *stream, idl_fasta **out)
{
    IDL_REQUIRE(path && codes && mask && out && cap_slots >= 1, "fasta_parse_pack: NULL argument");
    IDL_REQUIRE((dev_codes == nullptr) == (dev_mask == nullptr), "fasta_parse_pack: dev_codes and dev_mask go together");
    *out = nullptr;
    std::unique_ptr<idl_fasta> f(new idl_fasta());
    f->check = 1;
    bool empty = false;
    if (const int rc = map_file(path, &f->buf, &empty)) return rc;
    if (empty) return IDL_FALLBACK;                                   // (the general reader's one empty record)
    const uint8_t *buf = f->buf.data();
    const size_t size = f->buf.size();
    const int nt = (size > par_min_bytes() && size >= 64) ? n_threads() : 1;
    const double t_0 = now_ms();
    OnePass j{buf, size, codes, mask, cap_slots, dev_codes, dev_mask};
    j.timing = getenv("IDELUCS_INGEST_TIMING") != nullptr;
    // The file is cut into SLICES (IDELUCS_DEV=slices per thread, default 4) that the threads take from a counter: the threads of a
    // shared host do not run at one speed (a core's other hardware thread busy, a time slice lost: with one slice per thread they
    // finished between 5.4 and 7.6 ms), and the call ends with its slowest.  A slice owns the records whose header line starts in
    // it and its own region of the arenas, as a thread did.
    j.per_thread = idl::dev_env_int("slices", 4, 1, 64);
    j.ns = nt > 1 ? nt * j.per_thread : 1;
    j.outs.resize((size_t)j.ns);
    set_copy_schedule(j);
    std::vector<double> th_begin((size_t)nt, 0.0), th_end((size_t)nt, 0.0);
    std::atomic<int> next_slice{0};
    // the copies below are issued from worker threads: a new thread's current device is 0, so each worker adopts the CALLER's device
    // first (a rank of a multi-GPU job is bound to another one, and dev_codes / stream belong to it)
    int caller_dev = -1;
    if (dev_codes != nullptr && hipGetDevice(&caller_dev) != hipSuccess) caller_dev = -1;
    g_last_file_node = (nt > 1 && caller_dev >= 0 && !idl::dev_env("numa")) ? file_numa_node(buf, size) : -1;
    CpuBind bind = (nt > 1 && caller_dev >= 0) ? bind_for_device(caller_dev, nt, g_last_file_node) : CpuBind();
    if (g_last_file_node >= 0 && bind.node != g_last_file_node) bind = bind_for_device(caller_dev, nt);       // (too few CPUs open there: the device's node)
    g_last_bind_node = bind.node;
    j.sparse_mask = idl::dev_env_int("sparse_mask", 1, INT32_MIN, INT32_MAX) != 0;
    j.streams.assign(1, (hipStream_t)stream);
    if (dev_codes != nullptr && nt > 1 && caller_dev >= 0 && !open_copy_streams(j, (hipStream_t)stream, caller_dev)) {
        idl::set_error("fasta_parse_pack: hipStreamWaitEvent failed");
        return IDL_ERR_HIP;
    }

    parallel_for(nt, [&](int t) {
        if (j.timing) th_begin[(size_t)t] = now_ms();
        if (t > 0 && caller_dev >= 0 && hipSetDevice(caller_dev) != hipSuccess) { j.outs[0].copy_failed = 1; return; }
        for (int sl = next_slice.fetch_add(1); sl < j.ns; sl = next_slice.fetch_add(1)) one_pass_slice(j, t, sl);
        if (j.timing) th_end[(size_t)t] = now_ms();
    }, &bind);
    // the caller's stream continues when the other copy streams have drained
    for (size_t i = 1; i < j.streams.size(); ++i) {
        if (hipEventRecord(j.cs->done[i - 1], j.streams[i]) != hipSuccess || hipStreamWaitEvent((hipStream_t)stream, j.cs->done[i - 1], 0) != hipSuccess)
            j.outs[0].copy_failed = 1;
    }
    if (j.timing) report_timeline(j, t_0, th_begin, th_end, (hipStream_t)stream, bind.node);

    for (const FastOut &o : j.outs) {
        if (o.fallback) return IDL_FALLBACK;
        if (o.copy_failed) { idl::set_error("fasta_parse_pack: hipMemcpyAsync failed: %s", hipGetErrorString(hipGetLastError())); return IDL_ERR_HIP; }
        if (o.bad_kind != REC_OK) return report_bad_record(buf, o.bad_rec, o.bad_kind, o.bad_byte);      // the first failing record in file order decides
    }
    const size_t n = merge_slices(f.get(), j.outs, nt);
    if (j.timing) fprintf(stderr, "idl_fasta_parse_pack: one pass %.1f ms (%d threads, %zu records)\n", now_ms() - t_0, nt, n);
    *out = f.release();
    return IDL_OK;
}

int idl_fasta_arena_slots(const idl_fasta *f, int64_t *slot_off)
{
    IDL_REQUIRE(f && slot_off, "NULL argument");
    IDL_REQUIRE(f->arena_slot.size() == f->recs.size() + 1, "fasta_arena_slots: the handle does not come from idl_fasta_parse_pack");
    memcpy(slot_off, f->arena_slot.data(), f->arena_slot.size() * sizeof(int64_t));
    return IDL_OK;
}

int idl_fasta_arena_meta(const idl_fasta *f, int64_t *lengths, int64_t *slot_off, int64_t *min_len, int64_t *max_len)
{
    IDL_REQUIRE(f, "NULL argument");
    IDL_REQUIRE(f->arena_slot.size() == f->recs.size() + 1 && f->lengths.size() == f->recs.size(),
                "fasta_arena_meta: the handle does not come from idl_fasta_parse_pack");
    if (lengths && !f->lengths.empty()) memcpy(lengths, f->lengths.data(), f->lengths.size() * sizeof(int64_t));
    if (slot_off) memcpy(slot_off, f->arena_slot.data(), f->arena_slot.size() * sizeof(int64_t));
    if (min_len) *min_len = f->min_len;
    if (max_len) *max_len = f->max_len;
    return IDL_OK;
}

int64_t idl_fasta_arena_mask_flags(const idl_fasta *f, uint8_t *sent)
{
    if (!f || f->mask_sent.size() != f->recs.size()) return -1;
    if (sent && !f->mask_sent.empty()) memcpy(sent, f->mask_sent.data(), f->mask_sent.size());
    return f->n_mask_unsent;
}

void idl_fasta_close(idl_fasta *f) { delete f; }

void idl_ingest_release(void)
{
    std::shared_ptr<FileMap> m;
    { std::lock_guard<std::mutex> lk(g_map_mu); m.swap(g_map); g_map_key = MapKey{}; }
    if (m && m.use_count() == 1) m->unmap_inline = true;          // nobody else reads it: unmapped before this returns
}

int idl_fasta_names_high(const idl_fasta *f) { return f ? f->names_high : -1; }

int idl_fasta_sizes(const idl_fasta *f, int64_t *n_records, int64_t *total_bases, int64_t *total_slots,
                    int64_t *names_bytes)
{
    IDL_REQUIRE(f, "NULL handle");
    if (n_records) *n_records = (int64_t)f->recs.size();
    if (total_bases) *total_bases = f->total_bases;
    if (total_slots) *total_slots = f->total_slots;
    if (names_bytes) *names_bytes = f->names_bytes;
    return IDL_OK;
}

int idl_fasta_export(const idl_fasta *f, uint8_t *names, int64_t *name_off, int64_t *lengths,
                     uint8_t *bytes, int64_t *byte_off, uint8_t *codes, uint8_t *mask, int64_t *slot_off)
{
    IDL_REQUIRE(f, "NULL handle");
    IDL_REQUIRE(!codes || (mask && slot_off), "codes given without mask/slot_off");
    const int64_t n = (int64_t)f->recs.size();
    const uint8_t *buf = f->buf.data();
    std::vector<int64_t> boff((size_t)n + 1, 0), soff((size_t)n + 1, 0);
    int64_t noff = 0;
    for (int64_t i = 0; i < n; ++i) {
        const Rec &r = f->recs[(size_t)i];
        if (name_off) name_off[i] = noff;
        if (names && r.id_e > r.id_b) memcpy(names + noff, buf + r.id_b, r.id_e - r.id_b);
        noff += (int64_t)(r.id_e - r.id_b);
        if (lengths) lengths[i] = r.len;
        boff[(size_t)i + 1] = boff[(size_t)i] + r.len;
        soff[(size_t)i + 1] = soff[(size_t)i] + (r.len + 63) / 64;
    }
    if (name_off) name_off[n] = noff;
    if (byte_off) memcpy(byte_off, boff.data(), (size_t)(n + 1) * sizeof(int64_t));
    if (slot_off) memcpy(slot_off, soff.data(), (size_t)(n + 1) * sizeof(int64_t));
    if (!bytes && !codes) return IDL_OK;
    const int nt = (f->buf.size() > par_min_bytes() && n >= 2) ? n_threads() : 1;
    pack_records(f, 0, n, boff.data(), soff.data(), nt, bytes, codes, mask);
    return IDL_OK;
}

int idl_ingest_threads(void) { return n_threads(); }

int idl_ingest_numa_node(void) { return g_last_bind_node; }

int idl_ingest_file_node(void) { return g_last_file_node; }

int idl_ingest_probe_file_node(const char *path)
{
    if (path == nullptr) return -1;
    struct stat st;
    const int fd = open_regular(path, &st);
    if (fd < 0) return -1;
    int node = -1;
    if (st.st_size > 0) {
        void *m = mmap(nullptr, (size_t)st.st_size, PROT_READ, MAP_PRIVATE, fd, 0);
        if (m != MAP_FAILED) { node = file_numa_node((const uint8_t *)m, (size_t)st.st_size); munmap(m, (size_t)st.st_size); }
    }
    close(fd);
    return node;
}

int idl_ingest_cpu_plan(int device, int threads, int32_t *first_cpu, int32_t *n_cpus)
{
    IDL_REQUIRE(threads >= 1 && threads <= 256, "ingest_cpu_plan: threads outside 1..256");
    const CpuBind b = bind_for_device(device, threads);
    for (int t = 0; t < threads; ++t) {
        const cpu_set_t &c = b.of(t);
        int first = -1;
        if (b.on) for (int i = 0; i < CPU_SETSIZE; ++i) if (CPU_ISSET(i, &c)) { first = i; break; }
        if (first_cpu) first_cpu[t] = first;
        if (n_cpus) n_cpus[t] = b.on ? CPU_COUNT(&c) : 0;
    }
    return b.node;
}

int idl_fasta_pack_range(const idl_fasta *f, int64_t rec_lo, int64_t rec_hi, uint8_t *codes, uint8_t *mask)
{
    IDL_REQUIRE(f, "NULL handle");
    const int64_t n = (int64_t)f->recs.size();
    IDL_REQUIRE(rec_lo >= 0 && rec_lo <= rec_hi && rec_hi <= n, "record range outside the file");
    if (rec_lo == rec_hi) return IDL_OK;
    IDL_REQUIRE(codes && mask, "NULL buffer");
    // slot offset of rec_lo in the whole-file layout, then a local prefix over the range (balanced by cleaned bases)
    int64_t s0 = 0;
    for (int64_t i = 0; i < rec_lo; ++i) s0 += (f->recs[(size_t)i].len + 63) / 64;
    const int64_t m = rec_hi - rec_lo;
    std::vector<int64_t> boff((size_t)m + 1, 0), soff((size_t)m + 1, s0);
    for (int64_t i = 0; i < m; ++i) {
        const Rec &r = f->recs[(size_t)(rec_lo + i)];
        boff[(size_t)i + 1] = boff[(size_t)i] + r.len;
        soff[(size_t)i + 1] = soff[(size_t)i] + (r.len + 63) / 64;
    }
    const int nt = (boff[(size_t)m] > (int64_t)par_min_bytes() && m >= 2) ? n_threads() : 1;
    pack_records(f, rec_lo, m, boff.data(), soff.data(), nt, nullptr, codes, mask);
    return IDL_OK;
}

}  // extern "C"
