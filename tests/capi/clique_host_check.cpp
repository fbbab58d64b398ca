// Stand-alone check of hylight_amd/csrc/vq_clique_host.cpp (pure host code: the clique enumerator and the originals
// bookkeeping), meant to be built with the host sanitizers and run on its own - no GPU, no Python:
//   clang++ -std=c++17 -g -O1 -fsanitize=address,undefined -fno-sanitize-recover=all -D__HIP_PLATFORM_AMD__ \
//       -I<rocm>/include tests/capi/clique_host_check.cpp hylight_amd/csrc/vq_clique_host.cpp -o clique_host_check
//   ./clique_host_check tests/golden
// Feeds every tests/golden/fxK_<name>.graph.txt to the enumerator and compares with fxK_<name>.cliques.txt, then walks the
// originals functions.  Exit status 0 when everything matches.
#include <dirent.h>

#include <cstdio>
#include <fstream>
#include <sstream>
#include <string>

#include "../../hylight_amd/csrc/vq_internal.h"

static std::string slurp(const std::string &p) {
    std::ifstream f(p, std::ios::binary);
    std::stringstream s;
    s << f.rdbuf();
    return s.str();
}

int main(int argc, char **argv) {
    const std::string dir = argc > 1 ? argv[1] : "tests/golden";
    int bad = 0, seen = 0;
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
    printf("%d fixtures, %d problems\n", seen, bad);
    return bad || !seen ? 1 : 0;
}
