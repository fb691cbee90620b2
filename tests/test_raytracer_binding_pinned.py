"""The ray-tracer section of hip_kernels.HipKernels passes the library what it passed before it was restated on one gathered scene
(DESIGN 4.22): every public method over every medium, every refusal and its text, and which refusal wins where an input has two
defects, in both precisions. CPU only: raytracer_binding_pinned.Recorder records the calls and launches nothing."""
import json

import numpy as np
import torch

import raytracer_binding_pinned as BP


def test_binding_transcripts_are_the_recorded_ones(capsys):
    with open(BP.GOLDEN) as f:
        golden = json.load(f)
    got = BP.transcripts()
    form = BP.golden_form(got)
    refused = sum(1 for t in got.values() if t[-1].startswith("ValueError"))
    with capsys.disabled():
        print(f"\nraytracer binding: {len(got)} cases ran, {refused} of them refusals, {sum(len(t) - 1 for t in got.values())} recorded calls")
    assert sorted(form) == sorted(golden), "the methods that ran are not the recorded ones"
    for method, g in golden.items():
        now = form[method]
        # the same cases: none recorded that did not run, none run that is not recorded
        assert (now["cases"], now["names"]) == (g["cases"], g["names"]), f"{method}: the cases that ran are not the recorded {g['cases']}"
        names = [n for n in sorted(got) if n.split(" ")[1] == method]
        differ = [n for n, a, b in zip(names, now["each"].split(" "), g["each"].split(" ")) if a != b]
        for n in differ[:5]:
            print(f"{n}\n  now: {got[n]}")
        assert not differ, f"{method}: {len(differ)} transcripts differ from the recorded ones, the first: {differ[0]}"
        assert now == g, f"{method}: the transcripts differ from the recorded ones"


def test_every_method_and_two_defect_cases_are_covered():
    cases = BP.cases()
    assert {m for m, _, _ in cases.values()} == set(BP.METHODS)
    assert sum(1 for _, _, defects in cases.values() if len(defects) == 2) >= 4


def test_canonical_forms_tell_apart_what_must_differ():
    be = BP.Recorder(np.float64)
    t, u = torch.ones(3), torch.ones(3)
    be.reset(dict(tau=t, ssa=u))
    assert be.canon(1) != be.canon(True) and be.canon(1) != be.canon(1.0) and be.canon(None) == "None"
    assert be.canon(t) == "input tau" and be.canon(u) == "input ssa"
    assert be.canon(be.empty((2,))) != be.canon(be.zeros((2,)))
    assert be.canon(torch.zeros(2, dtype=torch.int64)) != be.canon(torch.ones(2, dtype=torch.int64))
    assert be.canon(np.zeros(2)) != be.canon(np.zeros(2, dtype=np.float32))
