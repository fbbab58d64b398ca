// Stand-alone check of vq_next_tables / vq_next_tables_check (hylight_amd/csrc/vq_superread.cpp, pure host): the lists
// findNextOverlaps reads of the vertices, built from what the merge and the clique step placed.  Meant to be built with the host
// sanitizers and run on its own - no GPU, no Python:
//   clang++ -std=c++17 -g -O1 -fsanitize=address,undefined -fno-sanitize-recover=all -D__HIP_PLATFORM_AMD__ \
//       -I<rocm>/include tests/capi/clique_next_host_check.cpp hylight_amd/csrc/vq_superread.cpp -o clique_next_host_check
//   ./clique_next_host_check
// The case is the first two lines of tests/test_vq_clique_next_model.py::test_tables_from_clique_map with one copied read.
// Exit status 0 when everything matches.
#include <cstdio>

#include "../../hylight_amd/csrc/vq_internal.h"

using namespace hlmi;

static int bad = 0;
static void expect(bool ok, const char *what) {
    if (!ok) { ++bad; printf("FAILED: %s\n", what); }
}
template <typename F> static bool refused(F f) {
    try { f(); } catch (...) { return true; }
    return false;
}

int main() {
    // super-read 0: vertices 0 at -7 and 1 at 3; super-read 1: vertices 1 at 0 and 2 at 12; vertices 3, 4 visited without a
    // list; vertex 5 copied as new read 2 (100 bases)
    const std::vector<VqMember> members{{0, 0, -7}, {1, 0, 3}, {1, 1, 0}, {2, 1, 12}};
    vqm::Rec lone{};
    lone.a = 5; lone.b = vqm::NONE; lone.len = 100; lone.id = 2;
    const VqNextTables t = vq_next_tables(6, members, 2, {93, 112}, {lone});
    expect(t.start == std::vector<uint32_t>{0, 1, 3, 4, 4, 4, 5}, "list bounds");
    expect(t.id == std::vector<uint32_t>{0, 0, 1, 1, 2}, "ids in ascending super-read order");
    expect(t.idx == std::vector<int32_t>{-7, 3, 0, 12, 0}, "signed indices");
    expect(t.copied == std::vector<uint8_t>{0, 0, 0, 0, 0, 1}, "copied flags");
    expect(t.len == std::vector<uint32_t>{93, 112, 100}, "lengths per new read");
    expect(!refused([&] { vq_next_tables_check(t, 6); }), "the tables pass their own check");
    expect(refused([&] { vq_next_tables_check(t, 7); }), "tables of another vertex count");
    VqNextTables x = t;
    x.id[4] = 3;
    expect(refused([&] { vq_next_tables_check(x, 6); }), "an id without a length");
    x = t;
    x.start[2] = 5;
    expect(refused([&] { vq_next_tables_check(x, 6); }), "list bounds that run backwards");
    expect(refused([&] { vq_next_tables(6, {{6, 0, 0}}, 2, {93, 112}, {}); }), "a member outside the vertices");
    expect(refused([&] { vq_next_tables(6, {{0, 2, 0}}, 2, {93, 112}, {}); }), "a member of a super-read that is not there");
    vqm::Rec twice = lone;
    twice.a = 1;
    expect(refused([&] { vq_next_tables(6, members, 2, {93, 112}, {twice}); }), "a copied read that is in a super-read");
    const VqNextTables none = vq_next_tables(0, {}, 0, {}, {});
    expect(none.start == std::vector<uint32_t>{0} && none.id.empty(), "no vertex at all");
    printf(bad ? "%d checks failed\n" : "clique_next_host_check: ok\n", bad);
    return bad ? 1 : 0;
}
