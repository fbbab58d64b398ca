"""GPU: the claims of tests/test_align_optimal.py on the rows the kernels write - optimal under the stated scores (claim A),
extensions that stopped where nothing more was to gain (B) and on a match (C) - next to equality with the oracle's file.
A kernel that differs from the oracle fails the equality; one that agrees with a wrong oracle fails a claim here.  One run
each with the default forms, with every certificate switched off (every task reaches a DP kernel), with the unpacked narrow
kernels, and with a run buffer of 3."""
import os
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import align_inputs as AI  # noqa: E402
import align_score as AS  # noqa: E402
from hylight_amd import api  # noqa: E402
from oracle import ava as OA  # noqa: E402
from test_gpu_ava_structured import VARIANTS  # noqa: E402

pytestmark = pytest.mark.gpu

FORMS = {
    "default": {},
    "no_certificates": {h: "1" for h in ("HLMI_NO_SHIFT_CERT", "HLMI_NO_GAP1_CERT", "HLMI_NO_GAP2_CERT", "HLMI_NO_SUFFIX_TRIM",
                                         "HLMI_NO_ONE_PIECE_CERT", "HLMI_NO_EXT_CERT")},
    "unpacked": {"HLMI_NARROW_UNPACKED": "1", "HLMI_NARROW_LONG_UNPACKED": "1"},
    "run_buf_3": {"HLMI_RUN_BUF_CAP": "3"},
}


class Sets:
    """the sets, the oracle's rows, the GPU's rows per form, and the claims per distinct text - each computed once"""

    def __init__(self, d):
        self.d = d
        self.exe = AS.compile_reference(d)
        self._set, self._want, self._judged, self.n = {}, {}, {}, 0

    def get(self, name):
        if name not in self._set:
            seqs = AI.SETS[name][0]()
            seqs, bounds = seqs if isinstance(seqs, tuple) else (seqs, None)
            self._set[name] = (seqs, bounds, AI.write_fasta(seqs, self.d / f"{name}.fa"))
        return self._set[name]

    @staticmethod
    def opts(mod, name, changes):
        short = AI.SETS[name][1] == "short"
        o = ((mod.ava_opts_short if short else mod.ava_opts_long) if mod is api else (mod.opts_short if short else mod.opts_long))()
        for k, v in changes.items():
            setattr(o, k, v)
        return o

    def want(self, name, **changes):
        key = (name, tuple(sorted(changes.items())))
        if key not in self._want:
            p = self.d / f"oracle{len(self._want)}.paf"
            OA.ava(self.get(name)[2], self.get(name)[2], p, self.opts(OA, name, changes))
            self._want[key] = open(p).read()
        return self._want[key]

    def got(self, name, **changes):
        self.n += 1
        p = self.d / f"gpu{self.n}.paf"
        api.ava(self.get(name)[2], self.get(name)[2], p, self.opts(api, name, changes))
        return open(p).read(), dict(api.last_stats())

    def judge(self, name, text, claims=None, **changes):
        """the claims on `text` (the GPU's rows); the same text under the same constants is judged once"""
        seqs, bounds, _ = self.get(name)
        claims = claims or AI.SETS[name][2]
        key = (name, claims, tuple(sorted(changes.items())), text)
        if key not in self._judged:
            o = self.opts(api, name, changes)
            reps, bad = AS.check_set(self.exe, text, seqs, o, self.d, claims, ties=AI.SETS[name][3], bounds=bounds, name=f"gpu_{name}")
            self._judged[key] = (reps, bad, AS.failure_text(self.exe, bad, o, self.d)[:3000] if bad else "")
        return self._judged[key]


@pytest.fixture(scope="module")
def sets(tmp_path_factory):
    return Sets(tmp_path_factory.mktemp("gpu_align"))


@pytest.fixture(scope="module")
def stats():
    return {}


@pytest.mark.parametrize("name", sorted(AI.SETS))
@pytest.mark.parametrize("form", list(FORMS))
def test_gpu_rows_are_optimal(sets, stats, monkeypatch, form, name):
    for k, v in FORMS[form].items():
        monkeypatch.setenv(k, v)
    text, st = sets.got(name)
    stats[(form, name)] = st
    reps, bad, why = sets.judge(name, text)
    rows, lossy, mean, worst = AS.loss_figures(reps)
    print(f"{form} {name}: {rows} rows judged; S < S* on {lossy}, mean loss {mean:.3f}, largest {worst}; tasks {st['align_tasks']}, "
          f"dp {st['align_tasks_dp']}, narrow {st['align_tasks_narrow']}, wide {st['align_tasks_wide']}, long {st['align_tasks_long']}")
    assert rows >= AI.SETS[name][4]
    assert not bad, why
    assert text == sets.want(name)


def test_noisy_rows_begin_and_end_on_a_match(sets):
    """Claim C measured on the GPU's rows of the noisy set, and what tests/test_align_optimal.py's test of this name asserts
    there (it has the figures and the cause): every row ends on a match; a row that does not begin on one has nothing to gain
    to its left."""
    text, _ = sets.got("noisy")
    reps, bad, _ = sets.judge("noisy", text, claims="C")
    print(f"noisy: claim C fails on {len(bad.get('C', []))} of {len(reps)} rows")
    AS.assert_first_fixed_point_alone(reps, bad.get("C", []))
    assert text == sets.want("noisy")


@pytest.mark.parametrize("variant", sorted(VARIANTS))
def test_planted_set_is_optimal_under_other_constants(sets, variant):
    text, _ = sets.got("planted", **VARIANTS[variant])
    reps, bad, why = sets.judge("planted", text, claims="0A", **VARIANTS[variant])
    assert len(reps) >= 20
    assert not bad, why
    assert text == sets.want("planted", **VARIANTS[variant])


def test_sets_reach_the_kernels_they_are_for(sets, stats, monkeypatch):
    if ("default", "long_block") not in stats:
        stats[("default", "long_block")] = sets.got("long_block")[1]
    st = stats[("default", "long_block")]
    assert st["align_tasks_narrow"] > 0 and st["align_tasks_wide"] > 0 and st["align_tasks_long"] > 0, st
    assert st.get("kernel_launches.align_long32", 0) >= 1 and st.get("kernel_launches.align_long", 0) >= 1, st
    for name in ("planted", "long_block"):
        if ("default", name) not in stats:
            stats[("default", name)] = sets.got(name)[1]
        if ("no_certificates", name) not in stats:
            for k, v in FORMS["no_certificates"].items():
                monkeypatch.setenv(k, v)
            stats[("no_certificates", name)] = sets.got(name)[1]
            for k in FORMS["no_certificates"]:
                monkeypatch.delenv(k)
        assert stats[("no_certificates", name)]["align_tasks_dp"] > stats[("default", name)]["align_tasks_dp"], name
