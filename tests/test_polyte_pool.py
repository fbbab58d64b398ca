"""CPU: hylight_amd/polyte_pool.py - the plan that deals clusters out to worker processes, the driver's refusals around
`--polyte_workers`, the share loop (what driver.polyte_native did inline) and the worker processes themselves, with
hylight_amd.polyte.run replaced by a stub: in this process by monkeypatch, in the children by a sitecustomize module this file
writes into a temporary directory on their PYTHONPATH (active only while HL_POLYTE_STUB_OUT is set)."""
import json
import os
import random
import signal
import subprocess
import sys
import time

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from hylight_amd import api, driver, polyte, polyte_pool  # noqa: E402
from hylight_amd.polyte_pool import plan  # noqa: E402


# -- plan ------------------------------------------------------------------------------------------------------------------
def test_plan_equal_sizes_alternate_over_the_bins():
    assert plan([5, 5, 5, 5], 2) == [[0, 2], [1, 3]]           # 0 -> bin 0, 1 -> bin 1, then the tie goes to the lowest bin again


def test_plan_one_giant_cluster_has_a_bin_to_itself():
    assert plan([1, 100, 2, 3], 2) == [[1], [0, 2, 3]]         # order 1, 3, 2, 0: everything after the giant fits beside it


def test_plan_more_bins_than_clusters_leaves_empty_bins():
    assert plan([4, 9], 4) == [[1], [0], [], []]


def test_plan_zero_clusters():
    assert plan([], 3) == [[], [], []]
    assert plan([], 1) == [[]]


def test_plan_ties_go_by_index_and_to_the_lowest_bin():
    # order 1, 2, 4 (the sevens, by index), then 0, 3 (the threes): loads 7/7/7 -> 10/7/7 -> 10/10/7
    assert plan([3, 7, 7, 3, 7], 3) == [[0, 1], [2, 3], [4]]
    assert plan([0, 0, 0], 2) == [[0, 1, 2], []]               # weightless clusters never raise a load: all stay in bin 0


def test_plan_refuses_no_bins():
    with pytest.raises(ValueError):
        plan([1], 0)


@pytest.mark.parametrize("seed", range(6))
def test_plan_properties(seed):
    rng = random.Random(seed)
    n, n_bins = rng.randint(1, 60), rng.randint(1, 9)
    sizes = [rng.choice([0, 1, 7, 7, 300, rng.randint(1, 10 ** 6)]) for _ in range(n)]
    bins = plan(sizes, n_bins)
    assert len(bins) == n_bins
    assert sorted(i for b in bins for i in b) == list(range(n))                 # a partition of range(n)
    assert all(b == sorted(b) for b in bins)                                    # every bin in directory order
    assert plan(list(sizes), n_bins) == bins                                    # the same input, the same plan
    loads = [sum(sizes[i] for i in b) for b in bins]
    # list scheduling: the bin that ends largest was the smallest when it took its last cluster, so at most the mean then
    assert max(loads) <= sum(sizes) / n_bins + max(sizes)


# -- the driver's refusals ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flags", [["--polyte_workers", "2"],
                                   ["--polyte_native", "--polyte_workers", "0"],
                                   ["--polyte_native", "--gpus", "8", "--polyte_workers", "3"]])
def test_polyte_workers_refusals(tmp_path, flags):
    with pytest.raises(SystemExit) as e:
        driver.main(["-l", str(tmp_path / "x.fq"), "-o", str(tmp_path / "OUT"), *flags])
    assert "--polyte_workers" in str(e.value)
    if "--gpus" in flags:
        assert "16" in str(e.value)
    assert not (tmp_path / "OUT").exists()


def test_polyte_workers_defaults_to_one():
    a = driver.build_parser().parse_args(["-l", "x.fq"])
    assert a.polyte_workers == 1
    driver.refuse_polyte_workers(a)
    a = driver.build_parser().parse_args(["-l", "x.fq", "--polyte_native", "--gpus", "8", "--polyte_workers", "2"])
    driver.refuse_polyte_workers(a)                                             # 16 processes: allowed


# -- the stub -----------------------------------------------------------------------------------------------------------------
def stub_run(p1, p2, **kw):
    """In place of polyte.run: the cluster's name decides.  `bad*`: the cluster's own data is wrong (after a contigs.fasta was
    begun); `state*`: the same as a library error of the cluster's; `fail*`: a library error that is nobody's data; `slow*`:
    a cluster that takes a minute; everything else: contigs.fasta from the name, one line on stdout."""
    folder = os.path.dirname(p1)
    name = os.path.basename(folder)
    assert os.getcwd() == folder and os.path.basename(p1) == f"{name}.1.fq" and os.path.basename(p2) == f"{name}.2.fq"
    assert (kw["min_overlap_len"], kw["min_overlap_len_EC"], kw["hap_cov"], kw["stddev"], kw["min_clique_size"], kw["edge1"],
            kw["edge2"]) == (50, 60, 10, 27, 2, 0.93, 1.0)
    with open("contigs.fasta", "w") as f:
        f.write(f">{name}\nACGT\n")
    print(f"stub {name} insert {float(kw['insert_size'])} readlen {float(kw['average_read_len'])}")
    if "bad" in name:
        raise ValueError("Unequal number of /1 and /2 reads")
    if "state" in name:
        raise api.HlmiError(-6, "no reads left")
    if "fail" in name:
        raise api.HlmiError(-3, "device lost")
    if "slow" in name:
        time.sleep(60)


SITECUSTOMIZE = '''
import os
if os.environ.get("HL_POLYTE_STUB_OUT"):
    import json, sys
    sys.path.insert(0, os.environ["HL_POLYTE_STUB_TESTS"])
    from hylight_amd import api, polyte
    import test_polyte_pool as T

    def init(device=-1, host_threads=0):
        with open(os.path.join(os.environ["HL_POLYTE_STUB_OUT"], f"init_{os.getpid()}.json"), "w") as f:
            json.dump([device, host_threads], f)

    api.init = init
    polyte.run = T.stub_run
'''


def make_tree(tmp_path, names_and_sizes):
    """tmp/fq_60/<name>/<name>.{1,2}.fq with the given total size -> (tmp, folders in sorted order)."""
    tmp = tmp_path / "tmp"
    for name, size in names_and_sizes:
        d = tmp / "fq_60" / name
        d.mkdir(parents=True)
        (d / f"{name}.1.fq").write_bytes(b"A" * (size // 2))
        (d / f"{name}.2.fq").write_bytes(b"A" * (size - size // 2))
    return tmp, polyte_pool.cluster_folders(tmp, 60)


def child_env(monkeypatch, tmp_path):
    hook = tmp_path / "hook"
    hook.mkdir()
    (hook / "sitecustomize.py").write_text(SITECUSTOMIZE)
    out = tmp_path / "stub_out"
    out.mkdir()
    monkeypatch.setenv("PYTHONPATH", str(hook) + os.pathsep + ROOT + (os.pathsep + os.environ["PYTHONPATH"] if os.environ.get("PYTHONPATH") else ""))
    monkeypatch.setenv("HL_POLYTE_STUB_OUT", str(out))
    monkeypatch.setenv("HL_POLYTE_STUB_TESTS", os.path.join(ROOT, "tests"))
    return out


def count_popen(monkeypatch):
    started = []
    real = subprocess.Popen

    def popen(*a, **k):
        p = real(*a, **k)
        started.append(p)
        return p
    monkeypatch.setattr(subprocess, "Popen", popen)
    return started


# -- the share loop, in this process ---------------------------------------------------------------------------------------------
def test_cluster_sizes_and_folders(tmp_path):
    tmp, folders = make_tree(tmp_path, [("10", 31), ("3", 8), ("21", 0)])
    assert [os.path.basename(f) for f in folders] == ["10", "21", "3"] and all(os.path.isabs(f) for f in folders)
    assert polyte_pool.cluster_sizes(folders) == [31, 0, 8]
    os.remove(f"{folders[0]}/10.2.fq")
    assert polyte_pool.cluster_sizes(folders) == [15, 0, 8]                     # a missing file counts nothing


def test_run_with_one_worker_is_the_loop_in_this_process(tmp_path, monkeypatch):
    tmp, folders = make_tree(tmp_path, [("1", 10), ("2", 20), ("bad7", 30), ("state8", 5), ("9", 40)])
    monkeypatch.setattr(polyte, "run", stub_run)
    started = count_popen(monkeypatch)
    cwd = os.getcwd()
    assert polyte_pool.run(folders, 1, 0, 16, 450, 150) is None
    assert not started and os.getcwd() == cwd
    for name in ("1", "2", "9"):
        d = tmp / "fq_60" / name
        assert (d / "contigs.fasta").read_text() == f">{name}\nACGT\n"
        assert (d / "log.txt").read_text() == f"stub {name} insert 450.0 readlen 150.0\n"
    d = tmp / "fq_60" / "bad7"                                                  # logged there, did not stop 9 and state8
    assert not (d / "contigs.fasta").exists()
    assert (d / "log.txt").read_text() == ("stub bad7 insert 450.0 readlen 150.0\n"
                                           "hylight_amd.polyte: Unequal number of /1 and /2 reads\n")
    d = tmp / "fq_60" / "state8"
    assert not (d / "contigs.fasta").exists()
    assert (d / "log.txt").read_text().endswith("hylight_amd.polyte: libhylight_mi error -6: no reads left\n")
    assert not [p for p in os.listdir(tmp) if p.startswith("polyte_share")]


def test_a_library_error_that_is_not_the_clusters_propagates(tmp_path, monkeypatch):
    tmp, folders = make_tree(tmp_path, [("1", 10), ("2fail", 20), ("3", 30)])
    monkeypatch.setattr(polyte, "run", stub_run)
    cwd = os.getcwd()
    with pytest.raises(api.HlmiError) as e:
        polyte_pool.run(folders, 1, 0, 16, 450, 150)
    assert e.value.code == -3 and os.getcwd() == cwd
    assert (tmp / "fq_60" / "1" / "contigs.fasta").exists() and not (tmp / "fq_60" / "3" / "log.txt").exists()


def test_driver_polyte_native_called_as_before_runs_in_this_process(tmp_path, monkeypatch):
    tmp, folders = make_tree(tmp_path, [("1", 10), ("2", 20)])
    monkeypatch.setattr(polyte, "run", stub_run)
    started = count_popen(monkeypatch)
    driver.polyte_native(str(tmp), 60, 450, 150)
    assert not started
    assert [(tmp / "fq_60" / n / "log.txt").read_text() for n in ("1", "2")] == [f"stub {n} insert 450.0 readlen 150.0\n" for n in "12"]


# -- worker processes ------------------------------------------------------------------------------------------------------------
def test_worker_entry_runs_its_share(tmp_path, monkeypatch):
    tmp, folders = make_tree(tmp_path, [("4", 10), ("5", 20), ("bad6", 30)])
    out = child_env(monkeypatch, tmp_path)
    share = tmp / "share.txt"
    share.write_text("".join(f + "\n" for f in folders[:1] + folders[2:]))
    r = subprocess.run([sys.executable, "-m", "hylight_amd.polyte_pool", "--share", str(share), "--device", "3", "--host_threads", "5",
                        "--insert_size", "450", "--average_read_len", "150"], cwd=ROOT, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    assert [json.load(open(out / p)) for p in os.listdir(out)] == [[3, 5]]
    assert (tmp / "fq_60" / "4" / "log.txt").read_text() == "stub 4 insert 450.0 readlen 150.0\n"
    assert not (tmp / "fq_60" / "5" / "log.txt").exists()                       # not in the share
    assert (tmp / "fq_60" / "bad6" / "log.txt").read_text().endswith("Unequal number of /1 and /2 reads\n")
    assert not (tmp / "fq_60" / "bad6" / "contigs.fasta").exists()


def test_worker_entry_reports_a_propagated_error(tmp_path, monkeypatch):
    tmp, folders = make_tree(tmp_path, [("fail1", 10)])
    child_env(monkeypatch, tmp_path)
    share = tmp / "share.txt"
    share.write_text(folders[0] + "\n")
    r = subprocess.run([sys.executable, "-m", "hylight_amd.polyte_pool", "--share", str(share)], cwd=ROOT, capture_output=True,
                       text=True, timeout=120)
    assert r.returncode == 1 and "device lost" in r.stderr and "HlmiError" in r.stderr


def test_three_workers_share_the_clusters_and_the_threads(tmp_path, monkeypatch):
    sizes = [("1", 50), ("2", 40), ("3", 30), ("4", 20), ("bad5", 10)]
    tmp, folders = make_tree(tmp_path, sizes)
    out = child_env(monkeypatch, tmp_path)
    monkeypatch.setattr(polyte, "run", stub_run)
    started = count_popen(monkeypatch)
    polyte_pool.run(folders, 3, 2, 16, 450, 150)
    assert len(started) == 2 and all(p.returncode == 0 for p in started)
    assert sorted(json.load(open(out / p)) for p in os.listdir(out)) == [[2, 5], [2, 5]]       # device 2, 16 // 3 threads each
    for name, _ in sizes:
        assert (tmp / "fq_60" / name / "log.txt").read_text().startswith(f"stub {name} insert 450.0 readlen 150.0\n")
        assert (tmp / "fq_60" / name / "contigs.fasta").exists() == (name != "bad5")
    bins = plan([s for _, s in sizes], 3)                                       # [[0], [1, 4], [2, 3]]
    assert bins == [[0], [1, 4], [2, 3]]
    for k in (1, 2):
        assert (tmp / f"polyte_share_{k}.txt").read_text() == "".join(folders[i] + "\n" for i in bins[k])
    assert not (tmp / "polyte_share_0.txt").exists()


def test_empty_bins_start_no_process(tmp_path, monkeypatch):
    tmp, folders = make_tree(tmp_path, [("1", 50), ("2", 40)])
    child_env(monkeypatch, tmp_path)
    monkeypatch.setattr(polyte, "run", stub_run)
    started = count_popen(monkeypatch)
    polyte_pool.run(folders, 8, 0, 4, 450, 150)
    assert len(started) == 1                                                   # bin 0 here, bin 1 in a child, six empty bins
    assert all((tmp / "fq_60" / n / "contigs.fasta").exists() for n in "12")
    started.clear()
    polyte_pool.run([], 4, 0, 4, 450, 150)
    assert not started


def test_a_failing_child_ends_the_step(tmp_path, monkeypatch):
    """Bin 1's cluster fails with an error that is not its own data, bin 2's would take a minute: run() ends bin 2's process,
    names bin 1 with its status and stderr, and starts nothing more."""
    tmp, folders = make_tree(tmp_path, [("1", 30), ("fail2", 20), ("slow3", 10)])
    child_env(monkeypatch, tmp_path)
    monkeypatch.setattr(polyte, "run", stub_run)
    started = count_popen(monkeypatch)
    t0 = time.time()
    with pytest.raises(polyte_pool.PoolError) as e:
        polyte_pool.run(folders, 3, 0, 16, 450, 150)
    assert time.time() - t0 < 30
    assert e.value.bin == 1 and e.value.status == 1
    assert "bin 1" in str(e.value) and "status 1" in str(e.value) and "device lost" in str(e.value)
    assert len(started) == 2                                                    # one per bin, none after the failure
    assert [p.returncode for p in started] == [1, -signal.SIGTERM]
    assert (tmp / "fq_60" / "1" / "contigs.fasta").exists()                     # this process's own share was run


def test_a_child_killed_by_a_signal_ends_the_step(tmp_path, monkeypatch):
    tmp, folders = make_tree(tmp_path, [("1", 30), ("slow2", 20)])
    child_env(monkeypatch, tmp_path)
    started = []
    real = subprocess.Popen

    def popen(*a, **k):
        p = real(*a, **k)
        started.append(p)
        return p

    def run_and_kill(p1, p2, **kw):                                             # this process's cluster: meanwhile the child dies
        stub_run(p1, p2, **kw)
        started[0].kill()
    monkeypatch.setattr(subprocess, "Popen", popen)
    monkeypatch.setattr(polyte, "run", run_and_kill)
    with pytest.raises(polyte_pool.PoolError) as e:
        polyte_pool.run(folders, 2, 0, 16, 450, 150)
    assert e.value.bin == 1 and e.value.status == -signal.SIGKILL and "signal 9" in str(e.value)
