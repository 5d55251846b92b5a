// Host-side timing of the FASTA readers on host arenas: no device, CPU only.  Three timings per repetition, each on a fresh mapping
// (idl_ingest_release between them, as bench.py does):
//   parse_pack   idl_fasta_parse_pack (the one-pass reader)
//   open+export  idl_fasta_open + idl_fasta_export of names, lengths, codes and mask
//   open+range   idl_fasta_open + idl_fasta_pack_range over the whole file
// Build (from idelucs_amd/csrc, the way the `asan` target links, but optimised and without a sanitizer):
//   g++ -std=c++17 -O3 -D__HIP_PLATFORM_AMD__ -I/opt/rocm/include host_ingest.cpp runtime.cpp ../../tools/time_host_ingest.cpp -o time_host_ingest -L/opt/rocm/lib -Wl,-rpath,/opt/rocm/lib -lamdhip64 -lpthread
// Run:  IDELUCS_THREADS=1 ./time_host_ingest FILE [reps, default 15]     (FILE in the page cache; one warm-up repetition is dropped)
// Prints one line per repetition and the medians.  To compare two builds, alternate short runs of both (A B A B ...) and pool
// each build's repetitions: a shared host drifts more between minutes than between builds.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <sys/stat.h>

#include <algorithm>
#include <chrono>
#include <vector>

#include "../include/idelucs_hip.h"

static double now_ms() { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

static void must(int rc, const char *what)
{
    if (rc != IDL_OK) { fprintf(stderr, "%s failed (%d): %s\n", what, rc, idl_last_error()); exit(1); }
}

int main(int argc, char **argv)
{
    if (argc < 2) { fprintf(stderr, "usage: %s file [reps]\n", argv[0]); return 2; }
    const char *path = argv[1];
    const int reps = argc > 2 ? atoi(argv[2]) : 15;
    struct stat st;
    if (stat(path, &st) != 0) { fprintf(stderr, "cannot stat %s\n", path); return 2; }
    const int64_t cap = (int64_t)st.st_size / 48 + 4096 * (int64_t)idl_ingest_threads() + 1024;
    std::vector<uint8_t> codes((size_t)cap * 16, 1), mask((size_t)cap * 8, 1);      // (touched: the arenas' page faults are not the reader's)
    std::vector<double> t[3];
    for (int rep = -1; rep < reps; ++rep) {
        double ms[3];
        idl_fasta *h = nullptr;
        double t0 = now_ms();
        must(idl_fasta_parse_pack(path, codes.data(), mask.data(), cap, nullptr, nullptr, nullptr, &h), "idl_fasta_parse_pack");
        ms[0] = now_ms() - t0;
        idl_fasta_close(h);
        idl_ingest_release();

        int64_t n = 0, bases = 0, slots = 0, nb = 0;
        t0 = now_ms();
        must(idl_fasta_open(path, 1, &h), "idl_fasta_open");
        must(idl_fasta_sizes(h, &n, &bases, &slots, &nb), "idl_fasta_sizes");
        if (slots > cap) { fprintf(stderr, "arenas too small\n"); return 1; }
        {
            std::vector<uint8_t> names((size_t)nb + 1);
            std::vector<int64_t> name_off((size_t)n + 1), lengths((size_t)n + 1), slot_off((size_t)n + 1);
            must(idl_fasta_export(h, names.data(), name_off.data(), lengths.data(), nullptr, nullptr, codes.data(), mask.data(), slot_off.data()), "idl_fasta_export");
        }
        ms[1] = now_ms() - t0;
        idl_fasta_close(h);
        idl_ingest_release();

        t0 = now_ms();
        must(idl_fasta_open(path, 1, &h), "idl_fasta_open");
        must(idl_fasta_sizes(h, &n, nullptr, nullptr, nullptr), "idl_fasta_sizes");
        must(idl_fasta_pack_range(h, 0, n, codes.data(), mask.data()), "idl_fasta_pack_range");
        ms[2] = now_ms() - t0;
        idl_fasta_close(h);
        idl_ingest_release();

        if (rep < 0) continue;
        printf("rep %2d: parse_pack %8.2f  open+export %8.2f  open+range %8.2f ms\n", rep, ms[0], ms[1], ms[2]);
        for (int k = 0; k < 3; ++k) t[k].push_back(ms[k]);
    }
    for (int k = 0; k < 3; ++k) std::sort(t[k].begin(), t[k].end());
    if (reps > 0)
        printf("median of %d (%d threads): parse_pack %.2f  open+export %.2f  open+range %.2f ms\n", reps, idl_ingest_threads(), t[0][(size_t)reps / 2],
               t[1][(size_t)reps / 2], t[2][(size_t)reps / 2]);
    return 0;
}
