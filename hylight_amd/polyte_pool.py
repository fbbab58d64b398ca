"""The native POLYTE step over several processes of one GPU (`driver --polyte_native --polyte_workers W`).

The reference runs its POLYTE lines with `xargs -i -P <threads>` (HyLight.py:245); a cluster's library calls are far too small
to fill the card, and clusters are independent: every file a cluster writes depends on its own directory alone (the labelling
shuffle is reseeded inside every call, the library keeps no state between calls that reaches an output).  So the clusters are
dealt out to W bins (`plan`: longest processing time first, by the size of the cluster's two read files); this process runs
bin 0, a fresh interpreter per further bin runs the others on the same device:

    python -m hylight_amd.polyte_pool --share FILE --device D --host_threads T --insert_size I --average_read_len L

FILE holds one cluster directory per line.  The children are started with subprocess.Popen - never forked from, nor a
replacement of, a process that has initialised the GPU.  A cluster's files are byte for byte the same whichever process ran it.
With one worker nothing is started: `run_share` in this process is the whole step.
"""
from __future__ import annotations

import argparse
import contextlib
import os
import subprocess
import sys
import time

from . import api

STDERR_TAIL = 2000       # bytes of a failed child's stderr quoted in the error


class PoolError(RuntimeError):
    """A worker process of the POLYTE step failed: `bin` is its bin, `status` its exit status (negative: the signal)."""

    def __init__(self, bin, status, stderr_tail):
        self.bin, self.status = bin, status
        how = f"was killed by signal {-status}" if status < 0 else f"exited with status {status}"
        super().__init__(f"POLYTE worker of bin {bin} {how}; the other workers were ended, nothing is retried.  "
                         f"Its stderr ends:\n{stderr_tail}")


def plan(sizes, n_bins):
    """Clusters -> bins, longest processing time first: the clusters in descending sizes[i] (ties: ascending index), each to the
    bin with the smallest load so far (ties: the lowest bin).  -> n_bins lists of indices, each ascending, so that a bin runs its
    clusters in directory order.  Deterministic; the largest load is at most the mean load plus the largest size."""
    if n_bins < 1:
        raise ValueError("need at least one bin")
    loads = [0] * n_bins
    bins = [[] for _ in range(n_bins)]
    for i in sorted(range(len(sizes)), key=lambda i: (-sizes[i], i)):
        b = min(range(n_bins), key=lambda k: (loads[k], k))
        loads[b] += sizes[i]
        bins[b].append(i)
    return [sorted(b) for b in bins]


def cluster_folders(tmp, size):
    """The cluster directories of tmp/fq_<size>/ in sorted order, absolute."""
    outdir2 = os.path.abspath(os.path.join(tmp, f"fq_{size}"))
    return [f"{outdir2}/{i}" for i in sorted(os.listdir(outdir2))]


def cluster_sizes(folders):
    """The weight of every cluster directory for `plan`: the bytes of <cid>.1.fq plus <cid>.2.fq (a missing file counts 0)."""
    def size(p):
        return os.path.getsize(p) if os.path.isfile(p) else 0
    return [size(f"{f}/{os.path.basename(f)}.1.fq") + size(f"{f}/{os.path.basename(f)}.2.fq")
            for f in (os.fspath(f).rstrip("/") for f in folders)]


def run_share(folders, insert_size, average_read_len):
    """HyLight.py:228-242 for the cluster directories `folders`, one after the other in this process: hylight_amd.polyte.run
    with the options of driver.polyte_lines, each cluster's output in its log.txt.  A cluster that fails on its own data
    (ValueError; HLMI_EINVAL, HLMI_ESTATE) is logged there and leaves no contigs.fasta; every other library error propagates."""
    from . import polyte
    cwd = os.getcwd()
    for folder in folders:
        folder = os.path.abspath(os.fspath(folder)).rstrip("/")
        i = os.path.basename(folder)
        try:
            os.chdir(folder)
            with open("log.txt", "w") as log, contextlib.redirect_stdout(log):
                try:
                    polyte.run(f"{folder}/{i}.1.fq", f"{folder}/{i}.2.fq", min_overlap_len=50, min_overlap_len_EC=60, hap_cov=10,
                               insert_size=insert_size, stddev=27, average_read_len=average_read_len, min_clique_size=2,
                               edge1=0.93, edge2=1.0)
                except (api.HlmiError, ValueError) as e:
                    if isinstance(e, api.HlmiError) and e.code not in (-1, -6):    # only what the cluster's own data causes
                        raise                                                      # (HLMI_EINVAL, HLMI_ESTATE) is the cluster's
                    log.write(f"hylight_amd.polyte: {e}\n")
                    if os.path.exists("contigs.fasta"):
                        os.remove("contigs.fasta")
        finally:
            os.chdir(cwd)


def _end(procs):
    """Terminate what still runs of `procs` ({bin: (Popen, stderr path)}) and reap it."""
    for p, _ in procs.values():
        if p.poll() is None:
            p.terminate()
    for p, _ in procs.values():
        try:
            p.wait(timeout=10)
        except subprocess.TimeoutExpired:
            p.kill()
            p.wait()


def _tail(path):
    try:
        with open(path, "rb") as f:
            return f.read()[-STDERR_TAIL:].decode(errors="replace")
    except OSError:
        return ""


def run(folders, workers, device, host_threads, insert_size, average_read_len, bins=None, first_bin=0, share_dir=None,
        poll_s=0.05):
    """The POLYTE step over `folders` with `workers` processes on GPU `device`.  workers == 1: run_share here, no children.
    Otherwise the folders are planned into `workers` bins; bin 0 runs here, every further non-empty bin in a child of its own
    with max(1, host_threads // workers) host threads.  The first child that exits non-zero or is killed ends the step: the
    others are terminated, nothing is retried, PoolError names its bin.
    `bins`: a plan made by the caller (lists of indices into `folders`, one per worker) in place of this call's own, `first_bin`
    the number of its first bin in the caller's numbering (StagePool.polyte: one plan over the bins of all ranks).
    `share_dir`: where the share files and the children's stderr go (default: tmp/, two levels above the first folder)."""
    folders = [os.path.abspath(os.fspath(f)).rstrip("/") for f in folders]
    if workers < 1:
        raise ValueError("need at least one worker")
    if bins is None:
        if workers == 1:
            return run_share(folders, insert_size, average_read_len)
        bins = plan(cluster_sizes(folders), workers)
    if len(bins) != workers:
        raise ValueError(f"{len(bins)} bins for {workers} workers")
    procs = {}
    if any(bins[1:]):
        share_dir = os.path.abspath(share_dir or os.path.dirname(os.path.dirname(folders[0])))
        env = dict(os.environ)                      # the children import this package wherever the parent found it
        pkg_parent = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
        env["PYTHONPATH"] = pkg_parent + (os.pathsep + env["PYTHONPATH"] if env.get("PYTHONPATH") else "")
    try:
        for k in range(1, workers):
            if not bins[k]:
                continue                            # an empty bin starts no process
            share = os.path.join(share_dir, f"polyte_share_{first_bin + k}.txt")
            with open(share, "w") as f:
                f.writelines(folders[i] + "\n" for i in bins[k])
            err = share[:-4] + ".err"
            with open(err, "wb") as ef:
                p = subprocess.Popen([sys.executable, "-m", "hylight_amd.polyte_pool", "--share", share, "--device", str(device),
                                      "--host_threads", str(max(1, host_threads // workers)), "--insert_size", repr(float(insert_size)),
                                      "--average_read_len", repr(float(average_read_len))], env=env, stderr=ef)
            procs[first_bin + k] = (p, err)
        run_share([folders[i] for i in bins[0]], insert_size, average_read_len)
        live = set(procs)
        while live:
            for b in sorted(live):
                code = procs[b][0].poll()
                if code is None:
                    continue
                live.discard(b)
                if code != 0:
                    _end(procs)
                    raise PoolError(b, code, _tail(procs[b][1]))
            if live:
                time.sleep(poll_s)
    finally:
        _end(procs)                                 # (an exception in here, this process's own share included)
    for _, err in procs.values():
        if os.path.getsize(err):                    # a child that succeeded may still have warned
            sys.stderr.write(_tail(err))


def build_parser():
    p = argparse.ArgumentParser(prog="python -m hylight_amd.polyte_pool", description="one worker of the native POLYTE step")
    p.add_argument("--share", required=True, help="file with one cluster directory per line")
    p.add_argument("--device", type=int, default=0)
    p.add_argument("--host_threads", type=int, default=1)
    p.add_argument("--insert_size", type=float, default=450)             # (polyte.run takes both as floats)
    p.add_argument("--average_read_len", type=float, default=250)
    return p


def main(argv=None):
    a = build_parser().parse_args(argv)
    with open(a.share) as f:
        folders = [line.rstrip("\n") for line in f if line.strip()]
    try:
        api.init(a.device, a.host_threads)
        run_share(folders, a.insert_size, a.average_read_len)
    except Exception as e:
        sys.stderr.write(f"hylight_amd.polyte_pool: {type(e).__name__}: {e}\n")
        return 1
    return 0


if __name__ == "__main__":
    sys.exit(main())
