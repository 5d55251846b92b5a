// ingest_threads.h -- where and how the FASTA reader's threads run: how many (CPU quota, ranks of the node), on which NUMA node
// (the file's pages, else the device's), and the pool that keeps them between calls.  Nothing here knows about FASTA bytes.
#pragma once
#include <pthread.h>
#include <sched.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <sys/mman.h>
#include <sys/syscall.h>
#include <unistd.h>

#include <algorithm>
#include <condition_variable>
#include <functional>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "common.h"
#include "dev_env.h"

namespace {

// CPUs the process may actually use: the cgroup's CPU quota (cgroup v2 cpu.max, v1 cfs quota / period) where one is set, else 0.
// The process's own cgroup comes from /proc/self/cgroup (without a cgroup namespace -- systemd, Slurm -- the limit sits
// in a nested directory, not in /sys/fs/cgroup itself); every level up to the root is read, the tightest quota counts.
int cgroup_cpus()
{
    auto quota_of = [](const std::string &dir, bool v2) -> double {
        long quota = -1, period = -1;
        if (v2) {
            if (FILE *f = fopen((dir + "/cpu.max").c_str(), "r")) {
                char q[32] = {0};
                if (fscanf(f, "%31s %ld", q, &period) == 2 && strcmp(q, "max") != 0) quota = atol(q);
                fclose(f);
            }
        } else {
            if (FILE *g = fopen((dir + "/cpu.cfs_quota_us").c_str(), "r")) { if (fscanf(g, "%ld", &quota) != 1) quota = -1; fclose(g); }
            if (FILE *g = fopen((dir + "/cpu.cfs_period_us").c_str(), "r")) { if (fscanf(g, "%ld", &period) != 1) period = -1; fclose(g); }
        }
        return (quota > 0 && period > 0) ? (double)quota / (double)period : 0.0;
    };
    std::string v2_path = "/", v1_path = "/";
    if (FILE *f = fopen("/proc/self/cgroup", "r")) {
        char line[1024];
        while (fgets(line, sizeof(line), f)) {
            line[strcspn(line, "\n")] = 0;
            const char *c1 = strchr(line, ':');
            const char *c2 = c1 ? strchr(c1 + 1, ':') : nullptr;
            if (!c2) continue;
            const std::string ctrl(c1 + 1, c2);
            if (ctrl.empty()) v2_path = c2 + 1;                                            // "0::/path"
            else if (ctrl == "cpu" || ctrl == "cpu,cpuacct" || ctrl == "cpuacct,cpu") v1_path = c2 + 1;
        }
        fclose(f);
    }
    double best = 0.0;
    auto walk = [&](const std::string &root, std::string rel, bool v2) {
        for (;;) {
            const double q = quota_of(root + (rel == "/" ? "" : rel), v2);
            if (q > 0.0 && (best == 0.0 || q < best)) best = q;
            if (rel == "/" || rel.empty()) break;
            const size_t cut = rel.find_last_of('/');
            rel = (cut == 0 || cut == std::string::npos) ? "/" : rel.substr(0, cut);
        }
    };
    walk("/sys/fs/cgroup", v2_path, true);
    walk("/sys/fs/cgroup/cpu", v1_path, false);
    return best > 0.0 ? (int)(best + 0.999) : 0;
}

// Reader threads.  IDELUCS_THREADS overrides.  Default (round 4, profiles/r04_ingest_threads.txt: the 1 GB cfg2 file on a 256-thread
// host whose cgroup grants 16 CPUs): parse + pack 11.0 ms with 16 threads, 8.2 with 32, 7.6 with 48-64, but with the H2D copies in
// flight 11.4 / 12.0 / 13.6 and ingest-to-features 17.9 / 14.3 / 15.3 -- the threads block in page faults and in the copy calls, so
// twice the CPU quota pays and more does not.  Hence min(32, hardware threads, 2 x cgroup quota), and THAT is shared out over the
// ranks of the node (LOCAL_WORLD_SIZE: every rank of a multi-GPU job reads the file itself).
int n_threads()
{
    if (const char *e = getenv("IDELUCS_THREADS")) { const int t = atoi(e); if (t >= 1 && t <= 256) return t; }
    static const int chosen = [] {
        int t = (int)std::thread::hardware_concurrency();
        if (t <= 0) t = 1;
        if (const int q = cgroup_cpus(); q > 0 && 2 * q < t) t = 2 * q;
        if (t > 32) t = 32;
        int ranks = 1;
        if (const char *e = getenv("LOCAL_WORLD_SIZE")) { const int r = atoi(e); if (r >= 1 && r <= 64) ranks = r; }
        t /= ranks;
        return t < 1 ? 1 : t;
    }();
    return chosen;
}

size_t par_min_bytes()                  // files smaller than this are handled by one thread
{
    if (const char *e = idl::dev_env("par_min")) return (size_t)atoll(e);
    return (size_t)1 << 22;
}

// ---- NUMA placement of the reader (round 5; VERDICT r4 #1a).  Two things have a place: the file's page-cache pages (1 GB read) and
// the pinned arenas (375 MB written, then read by the DMA engine) -- hipHostMalloc puts pinned memory on the node nearest to the
// current device (ROCr's default without hipHostMallocNumaUser).  Measured on the pool's 2-socket boxes (profiles/r05_ingest_numa.txt,
// 1 GB cfg2 file, 32 threads): with file and GPU on one node, parse + pack 8.2 ms unbound, 6.9 bound there, 14.6 bound to the other
// node; with the file on the other node than the GPU, ingest-to-features 14.4 ms beside the GPU and 10.8 beside the FILE -- reads
// across the socket link cost, posted writes hardly.  The threads of a job that copies to a device are therefore bound, for the
// job, to the node of the file's pages (file_numa_node below) and, when the file does not say, to the device's node (workers
// keep the binding, the caller's own is restored).  IDELUCS_DEV=numa=off switches it off, =device ignores the file, =<node> forces a node.
struct CpuBind {
    cpu_set_t set;                      // the node's CPUs open to this process
    std::vector<cpu_set_t> per_thread;  // thread i of a job: the hardware threads of ONE core, cores dealt round-robin over the node's L3 domains
    int node = -1;
    bool on = false;
    const cpu_set_t &of(int i) const { return per_thread.empty() ? set : per_thread[(size_t)i % per_thread.size()]; }
};

int first_cpu_of_list(const char *path)      // first number of a sysfs cpu list ("64-71,192-199" -> 64), -1 when unreadable
{
    FILE *f = fopen(path, "r");
    if (!f) return -1;
    int v = -1;
    if (fscanf(f, "%d", &v) != 1) v = -1;
    fclose(f);
    return v;
}

// OPT-IN (IDELUCS_DEV=numa_pin=1): one core per reader thread, spread over the L3 domains, instead of the node's whole CPU set for every
// thread.  Built because the pool's threads, woken where they last ran, finished between 4.6 and 8.7 ms where freshly created ones
// took 4.8 .. 6.1; measured on three boxes (gpurun_out/r05_c..e, kept as profiles/r05_ingest_ab.txt): the pinned threads do finish
// closer together (9.1 .. 11.9 against 5.4 .. 12.1 ms) but the LAST one no earlier, and every job starts 1.3 ms late -- a thread
// that may run on two CPUs only waits for them (deep idle, or somebody else's time slice) where the scheduler would have taken any
// idle CPU of the node.  Ingest-to-features 14.5 / 11.8 / 16.3 ms pinned against 13.5 / 11.6 / 16.3 node-wide: node-wide is the default.
void spread_over_cores(CpuBind *b)
{
    const char *e = idl::dev_env("numa_pin");
    if (!(e && atoi(e) == 1)) return;
    struct Core { int l3, first; cpu_set_t cpus; };
    std::vector<Core> cores;
    for (int c = 0; c < CPU_SETSIZE; ++c) {
        if (!CPU_ISSET(c, &b->set)) continue;
        char path[128];
        snprintf(path, sizeof(path), "/sys/devices/system/cpu/cpu%d/topology/thread_siblings_list", c);
        const int first = first_cpu_of_list(path);
        if (first < 0) return;                         // no topology to read: keep the node-wide set
        bool seen = false;
        for (Core &k : cores) if (k.first == first) { CPU_SET(c, &k.cpus); seen = true; break; }
        if (seen) continue;
        snprintf(path, sizeof(path), "/sys/devices/system/cpu/cpu%d/cache/index3/shared_cpu_list", c);
        Core k;
        k.first = first;
        k.l3 = first_cpu_of_list(path);
        CPU_ZERO(&k.cpus);
        CPU_SET(c, &k.cpus);
        cores.push_back(k);
    }
    if (cores.size() < 2) return;
    std::vector<int> l3s;
    for (const Core &k : cores) if (std::find(l3s.begin(), l3s.end(), k.l3) == l3s.end()) l3s.push_back(k.l3);
    std::vector<size_t> next(l3s.size(), 0);
    std::vector<std::vector<size_t>> by_l3(l3s.size());
    for (size_t i = 0; i < cores.size(); ++i) by_l3[(size_t)(std::find(l3s.begin(), l3s.end(), cores[i].l3) - l3s.begin())].push_back(i);
    for (size_t placed = 0, g = 0; placed < cores.size(); g = (g + 1) % l3s.size()) {
        if (next[g] < by_l3[g].size()) { b->per_thread.push_back(cores[by_l3[g][next[g]++]].cpus); ++placed; }
    }
}

bool parse_cpulist(const char *path, cpu_set_t *out)
{
    FILE *f = fopen(path, "r");
    if (!f) return false;
    char buf[4096] = {0};
    const size_t got = fread(buf, 1, sizeof(buf) - 1, f);
    fclose(f);
    if (got == 0) return false;
    CPU_ZERO(out);
    const char *p = buf;
    while (*p) {
        while (*p == ',' || *p == ' ' || *p == '\n') ++p;
        if (!*p) break;
        char *e = nullptr;
        const long a = strtol(p, &e, 10);
        if (e == p) return false;
        long b = a;
        p = e;
        if (*p == '-') { b = strtol(p + 1, &e, 10); if (e == p + 1) return false; p = e; }
        for (long c = a; c <= b && c < CPU_SETSIZE; ++c) if (c >= 0) CPU_SET((int)c, out);
    }
    return CPU_COUNT(out) > 0;
}

// the CPUs of the NUMA node device `dev` hangs off, within what this thread may run on; .on = false when there is nothing to do
CpuBind bind_for_device(int dev, int want_threads, int file_node = -1)
{
    CpuBind b;
    const char *env = idl::dev_env("numa");
    if (env && (strcmp(env, "off") == 0 || strcmp(env, "-1") == 0)) return b;
    int node = -1;
    if (env && *env >= '0' && *env <= '9') node = atoi(env);
    else if (file_node >= 0 && !(env && strcmp(env, "device") == 0)) node = file_node;      // beside the file (IDELUCS_DEV=numa=device: beside the GPU)
    else {
        char id[64] = {0};
        if (dev < 0 || hipDeviceGetPCIBusId(id, (int)sizeof(id) - 1, dev) != hipSuccess) return b;
        for (char *c = id; *c; ++c) if (*c >= 'A' && *c <= 'F') *c = (char)(*c - 'A' + 'a');
        char path[160];
        snprintf(path, sizeof(path), "/sys/bus/pci/devices/%s/numa_node", id);
        FILE *f = fopen(path, "r");
        if (!f) return b;
        if (fscanf(f, "%d", &node) != 1) node = -1;
        fclose(f);
    }
    if (node < 0) return b;                       // a single-node host (or a VM that does not say)
    char path[96];
    snprintf(path, sizeof(path), "/sys/devices/system/node/node%d/cpulist", node);
    cpu_set_t nodeset, mine;
    if (!parse_cpulist(path, &nodeset)) return b;
    if (sched_getaffinity(0, sizeof(mine), &mine) != 0) return b;
    CPU_AND(&b.set, &nodeset, &mine);
    // too few CPUs of that node are open to this process (a cpuset on the other socket): leave the threads where they are
    if (CPU_COUNT(&b.set) == 0 || (CPU_COUNT(&b.set) < CPU_COUNT(&mine) && CPU_COUNT(&b.set) * 2 < want_threads)) return b;
    b.node = node;
    const char *pin = idl::dev_env("numa_pin");
    if (CPU_EQUAL(&b.set, &mine) && !(pin && atoi(pin) == 1)) return b;     // already there (one node, or an outer binding): leave the threads alone
    b.on = true;
    spread_over_cores(&b);
    return b;
}

// The NUMA node that holds the page-cache pages of a mapped file, or -1.  64 pages spread over the mapping: those that are
// resident (mincore: no I/O is started for a cold file) are touched, so that they are in this process's page table, and asked for
// their node (move_pages with a NULL target only reports; some container runtimes refuse it: -1 then).  A node counts when it
// holds 3/4 of the resident samples and at least 48 of the 64 were resident.
// Why it matters (profiles/r05_ingest_numa.txt, a 2-socket box, GPU on node 0, 1 GB cfg2 file): reading the file across the
// socket link is what costs -- pages on node 0: reader on node 0 10.8 ms ingest-to-features, on node 1 20.0; pages on node 1:
// reader on node 0 (beside the GPU and the pinned arenas) 14.4 ms, on node 1 (beside the FILE, writing the arenas remotely)
// 10.8.  The reader therefore goes where the file is, and to the device's node only when the file does not say.
int file_numa_node(const uint8_t *map, size_t size)
{
    const long psz = sysconf(_SC_PAGESIZE);
    if (psz <= 0 || size < (size_t)psz * 256) return -1;
    constexpr int S = 64;
    void *pages[S];
    int status[S];
    int n = 0;
    for (int i = 0; i < S; ++i) {
        const size_t off = (size / S * (size_t)i) & ~((size_t)psz - 1);
        unsigned char vec = 0;
        if (mincore((void *)(map + off), (size_t)psz, &vec) != 0 || !(vec & 1)) continue;
        (void)*(volatile const uint8_t *)(map + off);
        pages[n++] = (void *)(map + off);
    }
    if (n < 48) return -1;
    if (syscall(SYS_move_pages, 0, (unsigned long)n, pages, (const int *)nullptr, status, 0) != 0) return -1;
    int count[64] = {0}, seen = 0;
    for (int i = 0; i < n; ++i) if (status[i] >= 0 && status[i] < 64) { ++count[status[i]]; ++seen; }
    for (int node = 0; node < 64; ++node) if (count[node] * 4 >= seen * 3 && seen >= 48) return node;
    return -1;
}

// The reader's threads, kept between calls (round 5; VERDICT r4 #1b).  A run calls parallel_for seven times per file (scan, validate,
// pack, export ...); with std::thread per call that was 31 thread creations each -- ~1 ms of the 8 ms parse at 32 threads, and
// every new thread's first HIP call sets up its device state again.  Workers sleep on a condition variable; a job is
// (generation, thread count, callable); the caller runs index 0 itself and waits for the others.  One job at a time (callers
// from several host threads take turns).  The pool is never destroyed (threads blocked at process exit are the kernel's to
// reap); a forked child starts with an empty pool (its parent's threads do not exist there).
class ReaderPool {
public:
    static ReaderPool &get()
    {
        std::lock_guard<std::mutex> lk(inst_mu());
        static const bool hooked = [] {       // fork: nobody holds the instance lock across it; the child drops the parent's pool
            pthread_atfork([] { inst_mu().lock(); }, [] { inst_mu().unlock(); }, [] { inst() = nullptr; inst_mu().unlock(); });
            return true;
        }();
        (void)hooked;
        if (inst() == nullptr) inst() = new ReaderPool();
        return *inst();
    }
    template <typename F>
    void run(int nt, F &&fn, const CpuBind *bind = nullptr)
    {
        std::lock_guard<std::mutex> one_job(job_mu_);
        std::function<void(int)> f = [&fn](int t) { fn(t); };
        cpu_set_t before;
        // the caller, for the length of the job: the node's whole set -- it usually runs there already, so nothing migrates (bound to
        // one core like the workers it started its share 1.3 ms late: sched_setaffinity away from the current CPU waits for the
        // migration thread)
        const bool rebind = bind != nullptr && bind->on && sched_getaffinity(0, sizeof(before), &before) == 0 &&
                            sched_setaffinity(0, sizeof(cpu_set_t), &bind->set) == 0;
        {
            std::unique_lock<std::mutex> lk(mu_);
            while ((int)th_.size() < nt - 1) {
                const int idx = (int)th_.size() + 1;
                th_.emplace_back([this, idx] { worker(idx); });
                th_.back().detach();
            }
            fn_ = &f;
            nt_ = nt;
            pending_ = nt - 1;
            if (bind != nullptr && bind->on) { bind_ = *bind; ++bind_gen_; }
            ++gen_;
        }
        cv_work_.notify_all();
        fn(0);
        {
            std::unique_lock<std::mutex> lk(mu_);
            cv_done_.wait(lk, [this] { return pending_ == 0; });
            fn_ = nullptr;
        }
        if (rebind) (void)sched_setaffinity(0, sizeof(before), &before);
    }
    int threads() const { return (int)th_.size(); }

private:
    static ReaderPool *&inst() { static ReaderPool *p = nullptr; return p; }      // (the parent's pool is leaked in a forked child on purpose)
    static std::mutex &inst_mu() { static std::mutex m; return m; }
    void worker(int idx)
    {
        uint64_t seen = 0, bound = 0;
        for (;;) {
            std::function<void(int)> *f = nullptr;
            cpu_set_t want;
            bool move = false;
            {
                std::unique_lock<std::mutex> lk(mu_);
                cv_work_.wait(lk, [&] { return gen_ != seen; });
                seen = gen_;
                if (idx < nt_) f = fn_;
                if (f != nullptr && bind_gen_ != bound) { want = bind_.of(idx); bound = bind_gen_; move = true; }
            }
            if (f == nullptr) continue;              // this job uses fewer threads
            if (move) (void)sched_setaffinity(0, sizeof(want), &want);      // (a worker keeps its node until a job names another)
            (*f)(idx);
            bool last;
            { std::lock_guard<std::mutex> lk(mu_); last = --pending_ == 0; }
            if (last) cv_done_.notify_one();
        }
    }
    std::mutex job_mu_, mu_;
    std::condition_variable cv_work_, cv_done_;
    std::vector<std::thread> th_;
    std::function<void(int)> *fn_ = nullptr;
    int nt_ = 0, pending_ = 0;
    uint64_t gen_ = 0, bind_gen_ = 0;
    CpuBind bind_;
};

template <typename F>
void parallel_for(int nt, F &&fn, const CpuBind *bind = nullptr)       // fn(thread index)
{
    if (nt <= 1) { fn(0); return; }
    static const bool pooled = [] { const char *e = idl::dev_env("reader_pool"); return !(e && atoi(e) == 0); }();
    if (pooled) { ReaderPool::get().run(nt, fn, bind); return; }
    // IDELUCS_DEV=reader_pool=0: a thread per call and index (round 4's form, kept for A/B runs); new threads inherit the caller's CPUs
    cpu_set_t before;
    const bool rebind = bind != nullptr && bind->on && sched_getaffinity(0, sizeof(before), &before) == 0 &&
                        sched_setaffinity(0, sizeof(cpu_set_t), &bind->set) == 0;
    std::vector<std::thread> th;
    for (int t = 1; t < nt; ++t) th.emplace_back([&fn, t, bind, rebind]() { if (rebind) (void)sched_setaffinity(0, sizeof(cpu_set_t), &bind->of(t)); fn(t); });
    fn(0);
    for (auto &x : th) x.join();
    if (rebind) (void)sched_setaffinity(0, sizeof(before), &before);
}

}  // namespace
