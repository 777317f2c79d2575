"""Volumes that take the re-check of csrc/skeleton.hip past what the eight pinned volumes of skeleton_oracle.py reach: more
candidate words than one grid of skel_round_kernel holds, the single-workgroup loop of skel_finish_kernel with thousands of
open words, multi-word rows and hundreds of rounds, and the carry from one word of a row into the next.

Every case is built in code from a seed and carries the conditions it exists for (`CONDITIONS`).  tests/test_skeleton_host.py
asserts them on the CPU from skeleton_oracle.round_model and the wrong re-check models, so a case that stops meeting a
condition fails there instead of quietly testing less; tests/test_skeleton_rounds_gpu.py runs the kernels on the cases."""
import numpy as np

import skeleton_oracle as so


def _noise(shape, density, seed):
    return (np.random.default_rng(seed).random(shape) < density).astype(np.uint8)


def make_case(name):
    if name == "many_words_short_chains":                    # isolated 2x2x3 blobs one voxel apart: two candidate rows each
        i, j, _ = np.indices((200, 200, 3))
        return ((i % 3 < 2) & (j % 3 < 2)).astype(np.uint8)
    if name == "slab_noise":
        return _noise((110, 110, 3), 0.95, 20261021)
    if name == "sheet_noise":
        return _noise((70, 70, 2), 0.9, 20261022)
    if name == "plate":
        return np.ones((2, 80, 130), dtype=np.uint8)
    if name == "plate_noise":
        return _noise((2, 80, 130), 0.92, 20261027)
    if name == "tree2":                                      # the `tree` volume with every coordinate doubled
        v = np.zeros((40, 48, 268), dtype=np.uint8)
        for a, b, r2 in so.TREE_STAMPS:
            so.stamp(v, tuple(2 * c for c in a), tuple(2 * c for c in b), 4 * r2)
        return v
    if name == "flat_axis0":
        return _noise((1, 90, 70), 0.9, 20261023)
    if name == "flat_axis1":
        return _noise((90, 1, 70), 0.9, 20261030)
    raise KeyError(name)


# case -> the conditions it must meet.  Keys:
#   shape                 the extents
#   words_per_row, tail   words of a row and voxels in its last word
#   min_words             more than this many candidate words in some sub-iteration
#   min_open, max_open    more than / at most this many words open after ROUND_LAUNCHES rounds in some / every sub-iteration
#   min_rounds            more than this many rounds in some sub-iteration
#   min_passes            at least this many passes
#   differs               wrong re-check models whose skeleton must differ from the definition's
CONDITIONS = {
    "many_words_short_chains": dict(shape=(200, 200, 3), min_words=so.ROUND_WAVES, max_open=0),
    "slab_noise": dict(shape=(110, 110, 3), min_words=so.ROUND_WAVES, min_open=2000, differs=("late_dropped",)),
    "sheet_noise": dict(shape=(70, 70, 2), min_open=100 * so.FINISH_WAVES, min_rounds=100, differs=("late_unchecked", "late_dropped")),
    "plate": dict(shape=(2, 80, 130), words_per_row=3, tail=2, min_open=0, min_rounds=100, differs=("no_carry",)),
    "plate_noise": dict(shape=(2, 80, 130), words_per_row=3, tail=2, min_open=0, differs=("no_carry",)),
    "tree2": dict(shape=(40, 48, 268), words_per_row=5, tail=12, min_passes=7, differs=("late_dropped",)),
    "flat_axis0": dict(shape=(1, 90, 70), min_open=0),
    "flat_axis1": dict(shape=(90, 1, 70), min_open=0),
}
CASES = tuple(CONDITIONS)
GUARDED = ("sheet_noise", "plate_noise", "many_words_short_chains")      # also run over dirty scratch with red zones


class Solved:
    """A case thinned by skeleton_oracle.skeletonize_memo: `volume`, `skeleton`, `passes` and the Trace of the run."""

    def __init__(self, name):
        self.name = name
        self.volume = make_case(name)
        self.trace = so.Trace()
        self.skeleton, self.passes = so.skeletonize_memo(self.volume, trace=self.trace)
        for a in (self.volume, self.skeleton, self.trace.kind, self.trace.pass_, self.trace.direction, self.trace.round):
            a.setflags(write=False)

    def peak(self, field):
        return max(getattr(s, field) for s in self.trace.subiterations)

    def figures(self):
        return (f"{self.name}: {self.volume.shape}, {int(self.volume.sum())} voxels in, {int(self.skeleton.sum())} out, "
                f"{self.passes} passes, at most {self.peak('words')} candidate words, {self.peak('rounds')} rounds, "
                f"{self.peak('open_words')} words open after round {so.ROUND_LAUNCHES}")


_cache = {}


def solved(name) -> Solved:
    """Computed once per process; callers must not modify the arrays."""
    if name not in _cache:
        _cache[name] = Solved(name)
    return _cache[name]


def describe_difference(case: Solved, got, limit=5) -> str:
    """What a failure needs to say to be acted on without a rerun: how many voxels differ from the oracle's skeleton, and for
    the first few (raster order) what the oracle did with them the last time they were candidates, and in which round."""
    got = np.asarray(got)
    if got.shape != case.skeleton.shape:
        return f"{case.name}: shape {got.shape} against {case.skeleton.shape}"
    where = np.argwhere(got != case.skeleton)
    if not len(where):
        return f"{case.name}: no voxel differs"
    t = case.trace
    lines = [f"{case.name}: {len(where)} voxels differ from the oracle ({int((got != 0).sum())} set against {int(case.skeleton.sum())}); "
             f"rounds after {so.ROUND_LAUNCHES} belong to skel_finish_kernel, k % 64 == 0 takes the carry from the word before"]
    for i, j, k in where[:limit].tolist():
        if not case.volume[i, j, k]:
            what = "is background in the input"
        elif t.kind[i, j, k] == 0:
            what = "was never a candidate"
        else:
            what = (f"was last a candidate in pass {t.pass_[i, j, k]}, direction {t.direction[i, j, k]}, decided in round "
                    f"{t.round[i, j, k]}, and the oracle {'deleted' if t.kind[i, j, k] == 2 else 'kept'} it")
        lines.append(f"  ({i}, {j}, {k}) [word {k // so.WORD}, bit {k % so.WORD}]: kernel {int(got[i, j, k])}, oracle "
                     f"{int(case.skeleton[i, j, k])}; it {what}")
    if len(where) > limit:
        lines.append(f"  ... and {len(where) - limit} more, the last at {tuple(where[-1].tolist())}")
    return "\n".join(lines)
