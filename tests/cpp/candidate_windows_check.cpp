// candidate_windows_check -- the windows of a list of loop candidates and a round's slice of them (scl_slam_amd/csrc/
// candidate_windows.hpp) on their own, without a GPU and under ASan + UBSan (tests/test_candidate_windows.py runs it).  round(first, m,
// lead) is compared with a plain restatement that concatenates the windows of those candidates one by one; the windows are made the
// way the keyframe store makes them (registration.hip, kf_window): keyframes key - search_num .. key + search_num of a trajectory,
// those that exist.  Exit status 0 and "candidate_windows_check: ok", or the first failed check and 1.
#include "candidate_windows.hpp"

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <vector>

namespace {

constexpr int kBatch = 32;                       // scl_engine::kIcpBatch: candidates per round
constexpr int kTrajectory = 40;                  // keyframes 0 .. 39 exist

#define CHECK(cond)                                                                                        \
    do {                                                                                                   \
        if (!(cond)) {                                                                                     \
            std::fprintf(stderr, "candidate_windows_check: %s:%d: %s\n", __FILE__, __LINE__, #cond);       \
            std::exit(1);                                                                                  \
        }                                                                                                  \
    } while (0)

const unsigned char kStore[kTrajectory] = {};    // keyframe k's cloud "lives" at kStore + k: the windows carry the pointer only

struct Window {                                  // one window, kept on its own: the restatement's unit
    std::vector<const void *> clouds;
    std::vector<int> counts;
    std::vector<float> poses;
};

// the window of `key`: entry i of its 2 * search_num + 1 poses goes with keyframe key - search_num + i, tagged so that no two
// entries of a call look alike
Window make_window(int tag, int key, int search_num)
{
    Window w;
    for (int i = -search_num; i <= search_num; ++i) {
        const long long k = (long long)key + i;
        if (k < 0 || k >= kTrajectory) continue;
        w.clouds.push_back(kStore + k);
        w.counts.push_back(100 + 3 * (int)k);
        for (int t = 0; t < 16; ++t) w.poses.push_back((float)(tag * 4096 + (i + search_num) * 16 + t));
    }
    return w;
}

void add(scl::CandidateWindows *cw, const Window &w)
{
    cw->add(w.clouds.data(), w.counts.data(), w.poses.data(), (int)w.clouds.size());
}

// keys at both ends of the trajectory, inside it and beyond it (no keyframe at all)
int key_of(int c)
{
    static const int keys[] = {0, 1, kTrajectory - 1, kTrajectory - 2, 17, kTrajectory + 5, 2, -4, kTrajectory, 23};
    return keys[c % (int)(sizeof keys / sizeof keys[0])];
}

void check_round(const scl::CandidateWindows &cw, const std::vector<Window> &windows, int first, int m, const Window *lead_window)
{
    scl::CandidateWindows lead;
    if (lead_window) add(&lead, *lead_window);
    const scl::CandidateWindows::Round r = cw.round(first, m, lead_window ? &lead : nullptr);
    // the restatement: the lead, then candidates first .. first + m - 1, one by one
    std::vector<const Window *> want;
    if (lead_window) want.push_back(lead_window);
    for (int c = 0; c < m; ++c) want.push_back(&windows[(size_t)(first + c)]);
    CHECK(r.jobs == (int)want.size());
    CHECK(r.first.size() == want.size() + 1);
    CHECK(r.first[0] == 0);
    int at = 0;
    for (size_t j = 0; j < want.size(); ++j) {
        CHECK(r.first[j] == at);
        CHECK(r.first[j + 1] >= r.first[j]);
        const Window &w = *want[j];
        CHECK(r.first[j + 1] - r.first[j] == (int)w.clouds.size());
        for (size_t i = 0; i < w.clouds.size(); ++i) {
            CHECK((size_t)at + i < r.clouds.size() && r.counts.size() == r.clouds.size() && r.poses.size() == 16 * r.clouds.size());
            CHECK(r.clouds[(size_t)at + i] == w.clouds[i]);
            CHECK(r.counts[(size_t)at + i] == w.counts[i]);
            CHECK(std::equal(w.poses.begin() + 16 * i, w.poses.begin() + 16 * (i + 1), r.poses.begin() + 16 * ((size_t)at + i)));
        }
        at += (int)w.clouds.size();
    }
    CHECK(r.first.back() == at);
    CHECK((int)r.clouds.size() == at && (int)r.counts.size() == at && r.poses.size() == 16 * (size_t)at);
}

void rounds_of(int n_candidates, int search_num)
{
    std::vector<Window> windows;
    scl::CandidateWindows cw;
    CHECK(cw.size() == 0 && cw.entries() == 0);
    size_t entries = 0;
    for (int c = 0; c < n_candidates; ++c) {
        windows.push_back(make_window(c + 1, key_of(c), search_num));
        add(&cw, windows.back());
        entries += windows.back().clouds.size();
        CHECK(cw.size() == c + 1 && (size_t)cw.entries() == entries);
        if (key_of(c) - search_num >= kTrajectory || key_of(c) + search_num < 0) CHECK(windows.back().clouds.empty());
    }
    const Window lead = make_window(0, 5, 0), no_lead_keyframe = make_window(0, kTrajectory + 1, 0);
    CHECK(lead.clouds.size() == 1 && no_lead_keyframe.clouds.empty());
    // the rounds of a call: kBatch candidates each, and the loop forms' one round of no candidate behind the lead
    for (int first = 0; first < n_candidates || first == 0; first += kBatch) {
        const int m = std::min(n_candidates - first, kBatch);
        for (const Window *l : {(const Window *)nullptr, &lead, &no_lead_keyframe}) check_round(cw, windows, first, m, l);
    }
    // any slice, not only a round's: one candidate, and all of them
    for (int c = 0; c < n_candidates; ++c) check_round(cw, windows, c, 1, c & 1 ? &lead : nullptr);
    check_round(cw, windows, 0, n_candidates, &lead);
}

void shortened_windows()
{
    // search_num 2: the window of key 0 has keyframes 0 .. 2, of key 1 0 .. 3, of the last key the last three; beyond: none
    CHECK(make_window(1, 0, 2).clouds.size() == 3 && make_window(1, 1, 2).clouds.size() == 4);
    CHECK(make_window(1, kTrajectory - 1, 2).clouds.size() == 3 && make_window(1, kTrajectory + 5, 2).clouds.empty());
    CHECK(make_window(1, kTrajectory, 2).clouds.size() == 2 && make_window(1, -4, 2).clouds.empty());
    const Window w = make_window(1, 0, 2);                             // the poses that go with the keyframes that exist: entries 2 .. 4
    CHECK(w.poses[0] == (float)(4096 + 2 * 16) && w.clouds[0] == kStore);
    scl::CandidateWindows cw;
    add(&cw, make_window(1, kTrajectory + 5, 1));                      // windows with no keyframe: zero entries, offsets equal
    add(&cw, make_window(2, kTrajectory + 9, 1));
    CHECK(cw.size() == 2 && cw.entries() == 0 && cw.first_of[1] == 0 && cw.first_of[2] == 0);
    const scl::CandidateWindows::Round r = cw.round(0, 2);
    CHECK(r.jobs == 2 && r.first.size() == 3 && r.first[1] == 0 && r.first[2] == 0 && r.clouds.empty());
}

}  // namespace

int main()
{
    for (int n_candidates : {0, 1, 31, 32, 33, 64, 65})
        for (int search_num : {0, 1, 2}) rounds_of(n_candidates, search_num);
    shortened_windows();
    std::puts("candidate_windows_check: ok");
    return 0;
}
