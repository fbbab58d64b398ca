// Stand-alone check of the pure host code of the super-read steps - hylight_amd/csrc/vq_clique_host.cpp (the clique
// enumerator) and hylight_amd/csrc/vq_superread.cpp (what the merge and the clique step share) -, meant to be built with the
// host sanitizers and run on its own - no GPU, no Python:
//   clang++ -std=c++17 -g -O1 -fsanitize=address,undefined -fno-sanitize-recover=all -D__HIP_PLATFORM_AMD__ \
//       -I<rocm>/include tests/capi/clique_host_check.cpp hylight_amd/csrc/vq_clique_host.cpp \
//       hylight_amd/csrc/vq_superread.cpp -o clique_host_check
//   ./clique_host_check tests/golden
// Feeds every tests/golden/fxK_<name>.graph.txt to the enumerator and compares with fxK_<name>.cliques.txt, then walks the
// originals functions and the shared pieces on cases worked out by hand (tests/vq_clique_model.py's place and filter_subreads
// give the same values on the same inputs).  Exit status 0 when everything matches.
#include <dirent.h>

#include <cstdio>
#include <fstream>
#include <sstream>
#include <string>

#include "../../hylight_amd/csrc/vq_internal.h"

using namespace hlmi;

static std::string slurp(const std::string &p) {
    std::ifstream f(p, std::ios::binary);
    std::stringstream s;
    s << f.rdbuf();
    return s.str();
}

static int bad = 0;
static void expect(bool ok, const char *what) {
    if (!ok) { ++bad; printf("FAILED: %s\n", what); }
}

// n forward reads of the given lengths (all 'A' at 'I') with ids 10, 11, ...
static VqGraphState graph_of(std::initializer_list<size_t> lens) {
    VqGraphState g;
    for (size_t len : lens) {
        g.id.push_back(10 + g.seq.size());
        g.seq.emplace_back(len, 'A');
        g.qual.emplace_back(len, 'I');
    }
    g.out.resize(g.seq.size());
    g.orient.assign(g.seq.size(), 1);
    return g;
}
static void add_edge(VqGraphState &g, uint32_t v1, uint32_t v2, int32_t pos1) {
    VqEdge e{};
    e.v1 = v1; e.v2 = v2; e.pos1 = pos1; e.ori1 = e.ori2 = 1;
    g.out[v1].push_back(e);
}
static uint16_t col(char b, char q) { return (uint16_t)((b << 8) | q); }

static void check_placement() {
    VqPlaced order;
    // a pair at pos1 0: the other read goes in FRONT of the base (an equal entry is not smaller), whichever way the edge is stored
    for (int stored_from_other = 0; stored_from_other < 2; ++stored_from_other) {
        VqGraphState g = graph_of({10, 12});
        if (stored_from_other) add_edge(g, 1, 0, 0); else add_edge(g, 0, 1, 0);
        const int64_t total = vq_place(g, {0, 1}, "check", order);
        expect(total == 12 && order == VqPlaced{{0, 1}, {0, 0}}, "pair at pos1 0");
        expect(vq_edge_info(g, 0, 1)->v1 == (stored_from_other ? 1u : 0u), "pair at pos1 0: the edge's read 1");
    }
    {   // the edge stored other -> base at pos1 7: the other read at -7, then everything 7 to the right; 10 + 7 + max(0, 12 - 7 - 10)
        VqGraphState g = graph_of({10, 12});
        add_edge(g, 1, 0, 7);
        const int64_t total = vq_place(g, {0, 1}, "check", order);
        expect(total == 17 && order == VqPlaced{{0, 1}, {7, 0}}, "negative offset and shift");
    }
    {   // four reads of 10, 1 and 2 both at 3: the later one goes in front; total 10 + (5 + 10 - 10)
        VqGraphState g = graph_of({10, 10, 10, 10});
        add_edge(g, 0, 1, 3); add_edge(g, 0, 2, 3); add_edge(g, 0, 3, 5);
        add_edge(g, 1, 2, 0); add_edge(g, 1, 3, 2); add_edge(g, 2, 3, 2);       // (the clique's other edges: never looked at)
        const int64_t total = vq_place(g, {0, 1, 2, 3}, "check", order);
        expect(total == 15 && order == VqPlaced{{0, 0}, {3, 2}, {3, 1}, {5, 3}}, "equal offsets in a clique of four");
    }
    {   // read 2 reaches the base only through its own list (2 -> 0 at 2: offset -2); of two 0 -> 1 the first counts, and
        // base -> other goes before other -> base.  -2, 0, 4 shifted by 2; total 10 + 2 + (4 + 10 - 10)
        VqGraphState g = graph_of({10, 10, 10});
        add_edge(g, 0, 1, 4); add_edge(g, 0, 1, 9); add_edge(g, 1, 0, 6); add_edge(g, 1, 2, 1); add_edge(g, 2, 0, 2);
        const int64_t total = vq_place(g, {0, 1, 2}, "check", order);
        expect(total == 16 && order == VqPlaced{{0, 2}, {2, 0}, {6, 1}}, "a member found through its own out-list");
        expect(vq_edge_info(g, 0, 1)->pos1 == 4 && vq_edge_info(g, 1, 0)->pos1 == 6 && vq_edge_info(g, 0, 2)->v1 == 2, "getEdgeInfo");
    }
    {   // no edge between 0 and 3: refused, not read past
        VqGraphState g = graph_of({10, 10, 10, 10});
        add_edge(g, 0, 1, 3); add_edge(g, 1, 3, 2);
        expect(vq_edge_info(g, 0, 3) == nullptr, "getEdgeInfo without an edge");
        int code = 0;
        try { vq_place(g, {0, 1, 3}, "check", order); } catch (const Error &e) { code = e.code; }
        expect(code == HLMI_EINVAL, "a missing edge is refused");
    }
}

static void check_filter() {
    // seven reads at offsets 0 .. 6 that end at 10, 11, 12, 15, 15, 13, 14 + 2 = 16; min_clique_size 2 keeps 2 * 2: the two
    // leftmost (0, 1; the base is one of them), then from the largest end down: 6 (16), and of 3 and 4 (both 15) the one
    // std::sort leaves last - up to 16 elements an insertion sort, which keeps their order: 4
    VqGraphState g = graph_of({10, 10, 10, 12, 11, 8, 10});
    const VqPlaced order{{0, 0}, {1, 1}, {2, 2}, {3, 3}, {4, 4}, {5, 5}, {6, 6}};
    expect(vq_filter_subreads(g, 4, 0, order) == VqPlaced{{0, 0}, {1, 1}, {4, 4}, {6, 6}}, "filter_subreads with two equal ends");
}

static void check_columns() {
    // consensus_pos.  Q0: p = 1, the base itself scores log10(0) and the other three tie at log10(1 / 3): the first of A, T, C,
    // G among them; 1 - (1/3) / 1 = 2/3 -> phred 1.76 -> 2 = '#'.  Q1: p = 0.794, own 0.206 < 0.265 each other: the same
    // winners; 1 - 0.2648 / 1 = 0.7352 -> 1.34 -> 1 = '"'
    for (int q = 0; q < 2; ++q) {
        const char want_q = q == 0 ? '#' : '"';
        expect(vq_consensus_pos("A", &q, 1) == col('T', want_q), "one A at Q0 / Q1");
        for (const char *b : {"C", "G", "T"}) expect(vq_consensus_pos(b, &q, 1) == col('A', want_q), "one C, G, T at Q0 / Q1");
    }
    const int q40[3] = {40, 40, 40};
    expect(vq_consensus_pos("AC", q40, 2) == col('N', '$'), "two different bases of equal quality");
    expect(vq_consensus_pos("NNN", q40, 3) == col('N', '$'), "all N");
    // one column on the host: read 0 forward at 0, read 1 forward at 1, read 2 REVERSED at 2 (TTACG reads CGTAA, its
    // qualities ABCDE read EDCBA).  Column 3 holds T/I of read 0, G/5 of read 1 and G/D of read 2; column 0 read 0 alone;
    // column 5 the last base of read 1 (T/7) over A/B of read 2
    VqGraphState g = graph_of({5, 5, 5});
    g.seq = {"ACGTA", "CCGTT", "TTACG"};
    g.qual = {"IIIII", "34567", "ABCDE"};
    g.orient[2] = 0;
    const vqc::Entry entries[3] = {{0, 0, 0}, {1, 1, 0}, {2, 2, 1}};
    const int ph3[3] = {'I' - 33, '5' - 33, 'D' - 33}, ph0[1] = {'I' - 33}, ph5[2] = {'7' - 33, 'B' - 33};
    expect(vq_consensus_column(g, entries, 3, 3) == vq_consensus_pos("TGG", ph3, 3), "column with a reversed member");
    expect(vq_consensus_column(g, entries, 3, 0) == vq_consensus_pos("A", ph0, 1), "column of one read");
    expect(vq_consensus_column(g, entries, 3, 5) == vq_consensus_pos("TA", ph5, 2), "column of two reads");
    expect(vq_n_rate_ok(4, 100) && !vq_n_rate_ok(5, 100) && !vq_n_rate_ok(0, 0), "test_N_rate");
}

static void check_lone_reads() {
    // reads 0 .. 4; 1 is in a super-read, 2 is too short, 3 has too many N, 4 is reverse: ids 7 and 8 go to 0 and 4
    VqGraphState g = graph_of({20, 20, 5, 20, 20});
    g.orient[4] = 0;
    const VqOriginalsDict first("check", true, nullptr);
    std::vector<vqm::Rec> recs;
    std::string subreads;
    const VqLoneCounts c = vq_lone_reads(g, first, {0, 1, 0, 0, 0}, {0, 0, 0, 1, 0}, 10, nullptr, 7, recs, subreads, nullptr);
    expect(c.short_reads == 1 && c.n_reads == 1 && c.trivial == 2 && c.trivial_reverse == 1, "lone reads: the counts");
    expect(recs.size() == 2 && recs[0].a == 0 && recs[0].id == 7 && recs[0].flags == 0 && recs[1].a == 4 && recs[1].id == 8 &&
           recs[1].flags == vqm::F_REV_A && recs[1].b == vqm::NONE && recs[1].len == 20, "lone reads: the records");
    expect(subreads == "7\t10:+:0:20\n8\t14:-:0:20\n", "lone reads: the lines");
    // with the subreads of an earlier iteration: read 4 (id 14, reverse) holds original 3 forward at 2 of length 6 ->
    // mirrored 20 - (2 + 6); read 0 (id 10) is diverted; a read without a line is refused
    VqOriginalsDict later("check", false, "mem");
    later.dict = vq_parse_subreads("14\t3:+:2:6\n", "mem");
    recs.clear(); subreads.clear();
    std::vector<uint32_t> diverted;
    const std::vector<uint8_t> divert{1, 0, 0, 0, 0};
    vq_lone_reads(g, later, {0, 1, 1, 1, 0}, {0, 0, 0, 0, 0}, 0, &divert, 0, recs, subreads, &diverted);
    expect(diverted == std::vector<uint32_t>{0} && recs.size() == 1 && subreads == "0\t3:-:12:6\n", "lone reads: diverted, mirrored");
    int code = 0;
    try { later.originals_of(g, 0); } catch (const Error &e) { code = e.code; }
    expect(code == HLMI_EINVAL, "a read without a line is refused");
    code = 0;
    try { VqOriginalsDict none("check", false, nullptr); } catch (const Error &e) { code = e.code; }
    expect(code == HLMI_EINVAL, "first_it off without a file is refused");
}

int main(int argc, char **argv) {
    const std::string dir = argc > 1 ? argv[1] : "tests/golden";
    int seen = 0;
    DIR *d = opendir(dir.c_str());
    if (!d) { fprintf(stderr, "cannot open %s\n", dir.c_str()); return 2; }
    while (dirent *e = readdir(d)) {
        const std::string name = e->d_name, tail = ".graph.txt";
        if (name.compare(0, 4, "fxK_") != 0 || name.size() < tail.size() || name.compare(name.size() - tail.size(), tail.size(), tail) != 0) continue;
        const std::string stem = name.substr(0, name.size() - tail.size());
        const hlmi::VqCliqueList got = hlmi::vq_enumerate_cliques(slurp(dir + "/" + name));
        const bool ok = got.text == slurp(dir + "/" + stem + ".cliques.txt");
        printf("%-28s %6zu cliques %s\n", stem.c_str(), got.off.size() - 1, ok ? "ok" : "DIFFERS");
        bad += !ok;
        ++seen;
    }
    closedir(d);
    for (const char *text : {"", "3", "3\n2\n0,1\n", "2\n2\n0,5\n5,0\n", "2\n2\n0,0\n0,0\n", "2\n4\n0,1\n0,1\n1,0\n1,0\n"}) {   // refused, not read past
        try { hlmi::vq_enumerate_cliques(text); ++bad; printf("accepted a bad graph\n"); } catch (const hlmi::Error &) {}
    }
    // originals: a line is read back as written; a forward and a reverse member; the mirror
    const auto dict = hlmi::vq_parse_subreads("7\t3:+:0:100\t4:-:20:50\n\n8\t3:+:5:100\n", "mem");
    std::string line;
    hlmi::vq_subreads_line(line, 7, dict.at(7));
    bad += line != "7\t3:+:0:100\t4:-:20:50\n";
    hlmi::VqOriginals m;
    hlmi::vq_originals_add(m, dict.at(7), true, false, 10, 150);
    hlmi::vq_originals_add(m, dict.at(8), false, false, 30, 150);         // original 3 is there already
    bad += !(m.size() == 2 && m.at(3).index == 10 && m.at(4).index == 30 && !m.at(4).forward);
    hlmi::VqOriginals r;
    hlmi::vq_originals_add(r, dict.at(7), false, false, 2, 150);
    bad += !(r.at(4).forward && r.at(4).index == 150 + 2 - (50 + 20));
    hlmi::vq_originals_mirror(r, 150);
    bad += !(!r.at(4).forward && r.at(4).index == 150 - (82 + 50));
    check_placement();
    check_filter();
    check_columns();
    check_lone_reads();
    printf("%d fixtures, %d problems\n", seen, bad);
    return bad || !seen ? 1 : 0;
}
