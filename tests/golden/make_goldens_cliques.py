"""Writes tests/golden/fxK_<name>.graph.txt and fxK_<name>.cliques.txt: small graphs in the format of graph.txt (vertex count,
edge-line count, then each edge as "u,v" and "v,u") and what the reference's own clique enumerator prints for them.

    python tests/golden/make_goldens_cliques.py /path/to/HaploConduct/quick-cliques/bin/qc

Run where the reference tree is; the fixtures it writes are committed, this script only documents how they were made.  The
enumerator picks its reader by the file name (a name holding ".graph" is read in another format), so every graph is handed to
it under the name the pipeline uses, graph.txt.  stdout only: the run times it reports go to stderr.
"""
import os
import random
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))


def gnp(n, p, seed):
    rng = random.Random(seed)
    return n, [(u, v) for u in range(n) for v in range(u + 1, n) if rng.random() < p]


def complete(vs):
    vs = list(vs)
    return [(vs[i], vs[j]) for i in range(len(vs)) for j in range(i + 1, len(vs))]


def shapes():
    yield "path6", 6, [(i, i + 1) for i in range(5)]
    yield "triangle_pendant", 4, [(0, 1), (1, 2), (0, 2), (2, 3)]
    yield "k5", 5, complete(range(5))
    yield "two_k4", 6, sorted(set(complete(range(4)) + complete(range(2, 6))))
    yield "star8", 8, [(0, i) for i in range(1, 8)]
    yield "k333", 9, [(u, v) for u in range(9) for v in range(u + 1, 9) if u // 3 != v // 3]
    yield "empty5", 5, []
    for seed in (1, 2, 3):
        yield (f"gnp60_s{seed}",) + gnp(60, 0.2, seed)
    yield ("gnp300",) + gnp(300, 0.02, 7)


def graph_text(n, edges):
    return f"{n}\n{2 * len(edges)}\n" + "".join(f"{u},{v}\n{v},{u}\n" for u, v in edges)


def stageb_graph_text():
    """graph.txt of the stage-b fixture - tests/golden/fxC_v3.savage over the reads tests/test_gpu_vq_graph.py synthesizes for
    its ids, merge_contigs 1 - by the model of tests/vq_graph_model.py."""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    sys.path.insert(0, ROOT)
    import vq_graph_model as G
    from test_gpu_vq_graph import _random_reads
    ov = os.path.join(HERE, "fxC_v3.savage")
    ids = sorted({int(l.split("\t")[k]) for l in open(ov) for k in (0, 1)})
    with tempfile.TemporaryDirectory() as d:
        fq = os.path.join(d, "singles.fastq")
        _random_reads(fq, ids, 4000, 1)
        G.graph(fq, ov, os.path.join(d, "out"), merge_contigs=1.0)
        return open(os.path.join(d, "out", "graph.txt")).read()


def main(qc):
    todo = [(name, graph_text(n, e)) for name, n, e in shapes()]
    todo.append(("stageb", stageb_graph_text()))
    for name, text in todo:
        with tempfile.TemporaryDirectory() as d:
            path = os.path.join(d, "graph.txt")
            with open(path, "w") as f:
                f.write(text)
            out = subprocess.run([qc, "--algorithm=degeneracy", f"--input-file={path}"], stdout=subprocess.PIPE,
                                 stderr=subprocess.DEVNULL, check=True).stdout
        with open(os.path.join(HERE, f"fxK_{name}.graph.txt"), "w") as f:
            f.write(text)
        with open(os.path.join(HERE, f"fxK_{name}.cliques.txt"), "wb") as f:
            f.write(out)
        print(name, len(text), len(out))


if __name__ == "__main__":
    main(sys.argv[1])
