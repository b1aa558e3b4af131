"""The inputs and the bound of tests/test_gpu_attn_ranges.py, checked on the CPU (tests/attn_range_ref.py
holds the generators, the fp64 reference, the tile-walk model and its two mutants).

For every case the GPU file runs:
  * the model meets its own criterion against fp64 (each row within 2 × its worst row, and that
    worst row below 5e-3: bf16's unit roundoff 2⁻⁸ = 3.9e-3 is the size of one rounding of P or O,
    a row is the RMS of about 128 of each, and the model reaches 4.2e-3 at most on these cases);
  * the hard inputs make the lazy rescale work under the case's own mask.  Of the rows that admit
    keys in at least two 64-key tiles (no other row can rescale after its first tile; with a
    window of 8 that is a row in four, with 3 valid keys none), at least 25 % (a) move their
    reference max with a non-empty accumulator, at least 25 % (b) take a lazy step of more than
    one log2 unit, at least 5 % (c) rescale while the old mass is 10 % .. 90 % of the final l, and
    some 32-row group has a tile at which some rows rescale and others do not;
  * both mutants (alpha not applied to O columns 96..127; alpha taken from the neighbouring row)
    fail the criterion on the hard inputs and pass it on the randn inputs of the same seed, where
    no row rescales at all: the suite's randn tests could not have seen either bug.

(c) cannot hold where a row's second tile must outweigh its first by the rescale threshold while
the first keeps 10 % of the mass, which the key counts rule out:
  band8, masked_band8   17 admitted keys: at most 16 before the move, and a move needs a key 2⁸
                        times the old maximum, so the old share is below 16 / (16 + 256) = 5.9 %.
  small_1part           65 keys: the second tile is the single key 64, one profile step δ above key
                        63.  A move needs δ > 8 log2 units, so the first tile's mass is its last
                        key's (Σ 2^(−8d) < 1.004) against 2⁸ for key 64: an old share of 0.4 %.
                        That δ takes a ramp of 460 nats; the case is in the table for its
                        one-part route and its ragged tiles.
Measured on these inputs (a / b / c, in % of the rows counted): small_3parts 50 / 63 / 9,
small_causal 36 / 50 / 9, band128 40 / 60 / 7, tail_split 50 / 67 / 24, masked_full 50 / 66 / 8,
decode_g4 50 / 62 / 6, extend_g2 50 / 62 / 16, cross_s200 44 / 44 / 7, band8 28 / 27 / 0.
Mutants on the hard inputs: worst row 0.5 .. 8e2 (relative), 17 .. 5600 rows over the bound;
on the randn inputs: the same worst row as the correct model, to the last digit."""
import pytest
import torch

import attn_range_ref as R

NO_RELEVANT = {"band8", "masked_band8", "small_1part"}      # (c) ruled out by the key counts (above)


def _mutant_err(case, hard, mutant):
    d = R.case_data(case, hard)
    w = R.tile_walk(d["q"], d["k"], d["v"], d["ok"], mutant=mutant)
    return R.row_err(w["out"], d["ref"]), d["bound"]


@pytest.mark.parametrize("name", list(R.CASES))
def test_model_meets_its_own_criterion(name):
    case = R.CASES[name]
    for hard in (True, False):
        d = R.case_data(case, hard)
        worst = float(d["model_err"].max())
        assert torch.isfinite(d["model"]).all() and torch.isfinite(d["ref"]).all()
        assert worst <= d["bound"] == R.MARGIN * worst
        assert worst < 5e-3, (name, hard, worst)
        if case.entry != "probs":
            assert bool(d["ok"].any(-1).all()) or case.entry == "masked", "a query without an admissible key"


@pytest.mark.parametrize("name", R.WALK_CASES)
def test_hard_inputs_make_the_rescale_work(name):
    c = R.conditions(R.case_data(R.CASES[name])["walk"])
    print(name, c)
    assert c["rows"] > 0
    assert c["a"] >= 0.25, c
    assert c["b"] >= 0.25, c
    assert c["c"] >= 0.05 or name in NO_RELEVANT, c
    assert c["mixed"], c
    randn = R.case_data(R.CASES[name], hard=False)["walk"]
    assert int(randn["rescale"].sum()) == 0, "a randn row rescales: pick another seed for the demonstration"


@pytest.mark.parametrize("mutant", [1, 2])
@pytest.mark.parametrize("name", R.WALK_CASES)
def test_mutants_fail_on_hard_inputs_and_pass_on_randn(name, mutant):
    case = R.CASES[name]
    err, bound = _mutant_err(case, True, mutant)
    assert float(err.max()) > bound, (name, mutant, float(err.max()), bound)
    err, bound = _mutant_err(case, False, mutant)
    assert float(err.max()) <= bound, (name, mutant, float(err.max()), bound)
    assert float(err.max()) == float(R.case_data(case, False)["model_err"].max())


def test_masked_rows_without_a_key_are_the_documented_ones():
    """Only the key-padding cases hold rows without an admissible key (3 or 37 valid keys under a
    band or none): reference and model give them the entry's documented uniform weights, so no row
    is left out of the criterion."""
    for name, case in R.CASES.items():
        if case.entry == "probs":
            continue
        empty = ~R.case_data(case)["ok"].any(-1)
        assert bool(empty.any()) == (name == "masked_band8"), name


def test_probs_inputs_span_the_range():
    d = R.case_data(R.CASES["probs"])
    G = d["q"].shape[1] // d["k"].shape[1]
    s = (d["q"].double() @ d["k"].double().repeat_interleave(G, 1).transpose(2, 3)) * R.SCALE
    spread = s.amax(-1) - s.amin(-1)
    assert float(spread.max()) > 40.0 and float((spread > 20.0).float().mean()) >= 0.5
