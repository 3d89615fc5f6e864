// The host-only plan of the global voxel map (scl_slam_amd/csrc/global_map_plan.hpp), a program of its own built under ASan + UBSan
// (Makefile: tests/cpp/global_map_plan_check).  It answers the commands tests/test_global_map_abi.py writes to its standard input, one
// answer line per command:
//   cap N                      capacity_for(N)
//   start H                    start_capacity(H)
//   grown C U                  grown_capacity(C, U)
//   probe C                    probe_limit(C)
//   load U C                   over_load(U, C) as 0 / 1
//   room U C                   room(U, C)
//   hash K                     hash_key(K)
//   key CX CY CZ               make_key
//   groups N MAXJOBS MAXPTS c0 .. c(N-1)      "first ... | offsets ..."
//   set E N, then E lines "robot index generation p0 .. p6" (the map's entries) and N lines of the same (the call's list, generation =
//       the store's now)      "bad: ..." or "ok a0 .. a(N-1) | item sign p0 .. p6 ; ..." (poses as hexadecimal floats)
//   remove E N, then E entry lines and N lines "robot index generation"    "bad: ..." or "ok | item sign p0 .. p6 ; ..."
#include <cinttypes>
#include <cstdio>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "global_map_plan.hpp"

using namespace scl::gmap;

static double read_double(std::istream &in)
{
    std::string t;
    in >> t;
    return std::strtod(t.c_str(), nullptr);                 // hexadecimal floats: every bit as the test wrote it
}

static void read_entries(std::istream &in, int count, Entries *entries)
{
    for (int i = 0; i < count; ++i) {
        KeyframeId id{}; Entry en{};
        unsigned long long gen = 0;
        in >> id.robot >> id.index >> gen;
        en.generation = gen;
        for (double &v : en.pose) v = read_double(in);
        (*entries)[id] = en;
    }
}

static void print_jobs(const std::vector<Job> &jobs)
{
    for (size_t j = 0; j < jobs.size(); ++j) {
        std::printf("%s%d %d", j ? " ; " : " ", jobs[j].item, jobs[j].sign);
        for (double v : jobs[j].pose) std::printf(" %a", v);
    }
    std::printf("\n");
}

int main()
{
    std::string cmd;
    while (std::cin >> cmd) {
        if (cmd == "cap") { unsigned long long n; std::cin >> n; std::printf("%llu\n", capacity_for(n)); }
        else if (cmd == "start") { unsigned long long h; std::cin >> h; std::printf("%llu\n", start_capacity(h)); }
        else if (cmd == "grown") { unsigned long long c, u; std::cin >> c >> u; std::printf("%llu\n", grown_capacity(c, u)); }
        else if (cmd == "probe") { unsigned long long c; std::cin >> c; std::printf("%d\n", probe_limit(c)); }
        else if (cmd == "load") { unsigned long long u, c; std::cin >> u >> c; std::printf("%d\n", over_load(u, c) ? 1 : 0); }
        else if (cmd == "room") { unsigned long long u, c; std::cin >> u >> c; std::printf("%llu\n", room(u, c)); }
        else if (cmd == "hash") { unsigned long long k; std::cin >> k; std::printf("%llu\n", hash_key(k)); }
        else if (cmd == "key") { long long x, y, z; std::cin >> x >> y >> z; std::printf("%llu\n", make_key(x, y, z)); }
        else if (cmd == "groups") {
            int n, max_jobs; long long max_points;
            std::cin >> n >> max_jobs >> max_points;
            std::vector<int> counts((size_t)n), first, offsets;
            for (int &c : counts) std::cin >> c;
            plan_groups(counts.data(), n, &first, &offsets, max_jobs, max_points);
            std::printf("first");
            for (int v : first) std::printf(" %d", v);
            std::printf(" | offsets");
            for (int v : offsets) std::printf(" %d", v);
            std::printf("\n");
        } else if (cmd == "set" || cmd == "remove") {
            int ne, n;
            std::cin >> ne >> n;
            Entries entries;
            read_entries(std::cin, ne, &entries);
            std::vector<int> robots((size_t)n), indices((size_t)n); std::vector<uint64_t> gens((size_t)n); std::vector<double> poses(7 * (size_t)n);
            for (int i = 0; i < n; ++i) {
                unsigned long long g;
                std::cin >> robots[(size_t)i] >> indices[(size_t)i] >> g;
                gens[(size_t)i] = g;
                if (cmd == "set") for (int k = 0; k < 7; ++k) poses[7 * (size_t)i + k] = read_double(std::cin);
            }
            std::vector<int> actions{-7}; std::vector<Job> jobs(1);          // a refusal leaves them as they are
            const char *bad = cmd == "set" ? plan_set(entries, robots.data(), indices.data(), poses.data(), gens.data(), n, &actions, &jobs)
                                           : plan_remove(entries, robots.data(), indices.data(), gens.data(), n, &jobs);
            if (bad) {
                if (actions.size() != 1 || actions[0] != -7 || jobs.size() != 1) { std::printf("bad AND outputs written\n"); return 1; }
                std::printf("bad: %s\n", bad);
                continue;
            }
            std::printf("ok");
            if (cmd == "set") for (int a : actions) std::printf(" %d", a);
            std::printf(" |");
            print_jobs(jobs);
        } else {
            std::fprintf(stderr, "unknown command %s\n", cmd.c_str());
            return 2;
        }
    }
    return 0;
}
