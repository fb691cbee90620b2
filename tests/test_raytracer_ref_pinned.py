"""The numpy restatement of the ray tracers against its recorded results (raytracer_pinned.py,
tests/golden/raytracer_ref_digests.json): every recorded case is recomputed and must give the same bits."""
import pytest

from raytracer_pinned import PINNED, CASES, digest, run


@pytest.mark.parametrize("kind", sorted({c["kind"] for c in CASES}))
def test_the_restatement_gives_the_recorded_bits(kind):
    wrong = []
    for case in CASES:
        if case["kind"] == kind:
            res = run(case)
            keys = PINNED["keysets"][case["keys"]]
            assert set(keys) <= set(res), (case["name"], sorted(set(keys) - set(res)))
            if digest(res, keys) != case["digest"]:
                wrong.append(case["name"])
    assert not wrong, wrong


def test_the_recorded_cases_cover_what_they_should():
    """both precisions, top_at_1 both ways, independent columns, a first photon or ray that is not 0, ranges > 1, a cap that binds,
    every form of aerosol, every sensor type and both flux sensors, and every module that the restatement once was"""
    def values(key, kinds=None):
        return {str(c.get(key)) for c in CASES if kinds is None or c["kind"] in kinds}
    for kinds in (("fw",), ("bw",), ("spectral_fw",), ("spectral_bw",)):
        assert values("dtype", kinds) == {"f64", "f32"} and values("top_at_1", kinds) == {"True", "False"}
        assert values("table", kinds) == {"True", "False"} and values("bg", kinds) == {"True", "False"}
        assert "6" in values("max_events", kinds) and len(values("first", kinds)) > 1
    for kinds in (("fw",), ("bw",)):
        assert values("aerosol", kinds) == {"none", "grid", "aloft", "both", "zeros"}
        assert {"raytracer_bg_ref", "raytracer_aer_ref"} < values("via", kinds)
    assert "True" in values("independent_column", ("fw",)) and "4" in values("ranges", ("bw",))
    used = {c["sensor"] for c in CASES if c["kind"] == "bw"}
    assert {PINNED["sensors"][s]["type"] for s in used} == {0, 1, 2, 3} and {"flux_up", "flux_dn"} <= used
    assert values("via") == {"raytracer_ref", "raytracer_bw_ref", "raytracer_bg_ref", "raytracer_aer_ref", "raytracer_spectral_ref",
                             "raytracer_bw_spectral_ref"}
    assert {"sw", "bw_solve", "spectral_sw", "render"} < values("kind")
