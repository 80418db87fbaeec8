"""The posterior classes of a fitted model against the truth measured by the join: one seed that
is not among the eight of tools/copy_spectrum_recovery.py, at its one setting (tests/repeat_recovery.py's: a 300 000-base
repeat genome, 60 000 reads), through tests/copy_spectrum_recovery.py, with both models.

The caps are twice the worst gap the tool recorded over seeds 1..8, per model (profiles/copy_spectrum_recovery.txt) -- the
margin of sections 6l and 6n: the worst of eight says little about the ninth.

  error cutoff   model and measured were 4 and 4 in eight of eight seeds with both models: the cap on their distance is 0.
  erroneous      |expected - observed| / observed: at most 0.00038 (basic), 0.00011 (repeats) over the eight.
  1-copy k-mers  over ALL keys the two totals are not one quantity and do not meet -- the model's copy classes count an
                 erroneous k-mer under the copy number of the k-mer it was misread from, the measured ones count genomic
                 k-mers only: gap 2.94 .. 3.02 with the repeat model, 4.89 .. 5.46 with the basic one -- so that gap is
                 printed and NOT asserted (a cap of 6 holds nothing; the finding is in 6am).  What is asserted in its
                 place is the like-for-like total compare returns: over the keys the model calls error-free (E_0 >= 0.99)
                 alone, at most 0.00563 with the repeat model.  The basic model has no copy numbers: its 0.30 there is
                 printed only.
  2 and >= 3 copies, like for like: at most 0.050 and 0.079 (repeats); printed, not asserted.
"""
import pytest

pytestmark = pytest.mark.gpu

SEED = 0
RECORDED_WORST = {   # profiles/copy_spectrum_recovery.txt, "largest gap", seeds 1..8
    "basic": {"error_cutoff": 0.0, "erroneous": 0.00038},
    "repeats": {"error_cutoff": 0.0, "erroneous": 0.00011, "error_free_copies_1": 0.00563},
}


@pytest.mark.parametrize("model", ["basic", "repeats"])
def test_posterior_classes_recover_the_joined_truth(hip_lib, model):
    from copy_spectrum_recovery import recover
    got = recover(SEED, model)
    held = RECORDED_WORST[model]
    print("%s: estimate %s; error cutoff model %s measured %s" % (model, " ".join("%.6g" % v for v in got["estimate"]),
                                                                  got["cutoff"][0], got["cutoff"][1]))
    for name, gap in got["gaps"].items():
        print("%-24s gap %.5f%s" % (name, gap, "  cap %.5f" % (2 * held[name]) if name in held else "  (not asserted)"))
    assert got["cutoff"][0] is not None and got["cutoff"][1] is not None
    for name, worst in held.items():
        assert got["gaps"][name] <= 2 * worst, (model, name, got["gaps"][name], 2 * worst)
