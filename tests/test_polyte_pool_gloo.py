"""CPU, world_size 2 over gloo: StagePool.polyte (hylight_amd/stage.py) - both ranks make the same plan over the cluster
directories, each runs its bins, the ranks exchange how it went - and serve()'s dispatch between POLYTE and stage calls.
hylight_amd.polyte.run is a stub in both ranks, the GPU job of the stage call the oracle-backed stand-in of
test_multirank_gloo.py."""
import json
import os
import sys

import pytest
import torch.multiprocessing as mp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SIZES = [("10", 500), ("21", 90), ("3", 300), ("40", 80), ("7", 410), ("9", 20)]       # in sorted directory order


def _rank(rank, world, port, tmp, fa, fail):
    import torch.distributed as dist
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from hylight_amd import api, polyte
    from hylight_amd.stage import StagePool
    from test_multirank_gloo import patch_product_with_oracle_job
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    patch_product_with_oracle_job()

    def stub(p1, p2, **kw):
        name = os.path.basename(os.path.dirname(p1))
        with open("ran_by.txt", "a") as f:                     # appended: a cluster run twice would show
            f.write(f"{rank}\n")
        if fail and rank == 1 and name == fail:
            raise api.HlmiError(-3, "device lost")
        with open("contigs.fasta", "w") as f:
            f.write(f">{name}\nACGT\n")

    polyte.run = stub
    pool = StagePool(rank, world)
    result = {"error": None}
    try:
        if rank == 0:
            pool.polyte(tmp, 60, 450, 150, 1)
            pool.stage(fa, fa, 2, os.path.join(tmp, "after.paf"), 1000, 2, 0.95)
        else:
            pool.serve()
    except Exception as e:
        result["error"] = f"{type(e).__name__}: {e}"
    result.update(calls=pool.calls, broken=pool.broken)
    if rank == 0:
        pool.shutdown()
    with open(os.path.join(tmp, f"result{rank}.json"), "w") as f:
        json.dump(result, f)
    dist.destroy_process_group()


def _spawn(tmp_path, fail):
    from hylight_amd import launch, polyte_pool, simulate as S
    tmp = tmp_path / "tmp"
    for name, size in SIZES:
        d = tmp / "fq_60" / name
        d.mkdir(parents=True)
        (d / f"{name}.1.fq").write_bytes(b"A" * (size // 2))
        (d / f"{name}.2.fq").write_bytes(b"A" * (size // 2))
    reads, _ = S.simulate_reads(seed=71, n_strains=2, genome_len=8000, n_reads=14, mean_len=3000, min_len=2000, max_len=5000)
    fa = str(tmp_path / "s1.fa")
    S.write_fasta(reads, fa)
    mp.spawn(_rank, args=(2, launch.free_port(), str(tmp), fa, fail), nprocs=2, join=True)
    folders = polyte_pool.cluster_folders(tmp, 60)
    assert [os.path.basename(f) for f in folders] == [n for n, _ in SIZES]
    bins = polyte_pool.plan(polyte_pool.cluster_sizes(folders), 2)
    return tmp, folders, bins, [json.load(open(tmp / f"result{r}.json")) for r in range(2)]


def test_two_ranks_share_the_clusters_by_the_plan(tmp_path):
    tmp, folders, bins, results = _spawn(tmp_path, None)
    assert bins == [[0, 1, 3, 5], [2, 4]]                      # 500 | 410 + 300 | then 90, 80, 20 to the lighter rank 0
    assert [r["error"] for r in results] == [None, None]
    ran = [open(os.path.join(f, "ran_by.txt")).read().split() for f in folders]
    assert all(len(r) == 1 for r in ran)                       # every cluster exactly once
    assert [[i for i, r in enumerate(ran) if r == [str(k)]] for k in range(2)] == bins
    assert all(os.path.exists(os.path.join(f, "contigs.fasta")) and os.path.exists(os.path.join(f, "log.txt")) for f in folders)
    # the stage call after it went through serve()'s dispatch on rank 1, and was merged on rank 0
    assert os.path.getsize(tmp / "after.paf") > 0
    assert [r["calls"] for r in results] == [2, 2] and not any(r["broken"] for r in results)


def test_a_failure_on_rank_one_is_raised_on_rank_zero(tmp_path):
    tmp, folders, bins, results = _spawn(tmp_path, "3")        # cluster 3 is in rank 1's bin
    assert 2 in bins[1]
    assert results[0]["error"].startswith("RuntimeError: POLYTE step failed on rank 1") and "device lost" in results[0]["error"]
    assert results[0]["broken"] and results[1]["broken"] and results[0]["calls"] == 0
    assert not (tmp / "after.paf").exists()
    ran = [open(os.path.join(f, "ran_by.txt")).read().split() if os.path.exists(os.path.join(f, "ran_by.txt")) else [] for f in folders]
    assert [ran[i] for i in bins[0]] == [["0"]] * 4            # rank 0 finished its own share before it heard
    assert ran[2] == ["1"] and ran[4] == []                    # rank 1 stopped at the failing cluster
