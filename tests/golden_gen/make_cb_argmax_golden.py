"""TEST INFRASTRUCTURE.  Generates tests/golden/cb/argmax_nonfinite.npz by calling the UNMODIFIED reference
get_model_actions (reagent/training/cb/utils.py:113-139, randomize_ties = False; through oracle/stubs.py plus the shims of
make_cb_golden._install) on rows of scores with NaN, +inf and -inf among present and absent arms.  Run where the reference
tree is present:
    python tests/golden_gen/make_cb_argmax_golden.py            (writes the fixture)
    python tests/golden_gen/make_cb_argmax_golden.py --check    (regenerates it and compares with the committed file)

The fixture is data only.  Layout, for A in GROUPS (rows of A arms):
    a<A>_scores [R, A] float32, a<A>_mask [R, A] bool,
    a<A>_actions_masked [R, 1] int64    the reference's answer under the mask,
    a<A>_actions_plain  [R, 1] int64    its answer without a mask (torch.argmax).
The rows of three arms are named ones (NAMED: what each is there for) followed by EVERY row over the values
(-inf, 1, +inf, NaN) under EVERY mask, the empty one included: 64 x 8 rows.  The rows of five arms are named ones only.
"""
import itertools
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
for _p in (ROOT, os.path.dirname(os.path.abspath(__file__))):
    if _p not in sys.path:
        sys.path.insert(0, _p)

from make_cb_golden import _install, _np  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "cb")
NAME = "argmax_nonfinite"
INF, NAN = float("inf"), float("nan")

# (scores, mask, what the row is there for)
NAMED = [
    ([-INF, -INF, -INF], [0, 1, 1], "all present arms -inf"),
    ([-INF, -INF, 0.0], [0, 1, 0], "the one present arm -inf, a number on an absent arm"),
    ([0.0, -INF, NAN], [0, 1, 0], "the one present arm -inf, a NaN on an absent arm"),
    ([1.0, NAN, 3.0], [1, 1, 1], "a NaN among present arms"),
    ([1.0, NAN, 3.0], [1, 0, 1], "a NaN on an absent arm only"),
    ([NAN, 2.0, NAN], [0, 1, 1], "the first NaN absent, the second present"),
    ([NAN, 2.0, NAN], [0, 1, 0], "NaNs on absent arms only"),
    ([1.0, INF, INF], [1, 1, 1], "a tie of +inf"),
    ([1.0, INF, INF], [1, 0, 1], "a tie of +inf, its lower arm absent"),
    ([NAN, 5.0, 1.0], [1, 1, 1], "a NaN first"),
    ([NAN, 5.0, 1.0], [0, 1, 1], "a NaN first, absent"),
    ([2.0, 2.0, NAN], [1, 1, 0], "a tie of numbers, a NaN absent"),
    ([2.0, 2.0, NAN], [1, 1, 1], "a tie of numbers before a NaN"),
    ([-INF, -INF, 1.0], [1, 1, 1], "a tie of -inf below a number"),
    ([-INF, -INF, -INF], [1, 1, 1], "a tie of -inf, all present"),
    ([3.0, -INF, INF], [1, 1, 0], "+inf absent"),
    ([3.0, -2.0, 7.0], [0, 0, 0], "no arm present"),
    ([NAN, INF, -INF], [0, 0, 0], "no arm present, nothing finite"),
    ([-3.0, -1.0, -2.0], [1, 1, 1], "negative numbers"),
    ([-3.0, -1.0, -2.0], [1, 0, 1], "negative numbers, the largest absent"),
]
NAMED5 = [
    ([-INF, NAN, -INF, 4.0, NAN], [1, 0, 1, 1, 0], "NaNs absent, a number behind two -inf"),
    ([-INF, NAN, -INF, 4.0, NAN], [1, 0, 1, 0, 0], "only -inf present, between absent NaNs"),
    ([-INF, NAN, -INF, 4.0, NAN], [1, 0, 1, 1, 1], "the last arm's NaN present"),
    ([0.5, INF, -INF, INF, 0.5], [1, 0, 1, 1, 1], "a tie of +inf, its lower arm absent"),
    ([0.5, -INF, -INF, -INF, 0.5], [0, 1, 1, 1, 0], "a tie of -inf alone present, arm 0 absent"),
    ([0.5, -INF, 0.25, -INF, 0.5], [0, 1, 1, 1, 1], "a number between two -inf"),
    ([-1e38, -INF, -3e38, -INF, -INF], [0, 1, 1, 1, 1], "the most negative numbers against -inf"),
    ([7.0, 7.0, 7.0, 7.0, 7.0], [0, 0, 0, 0, 1], "the last arm alone"),
    ([7.0, 7.0, 7.0, 7.0, 7.0], [0, 0, 0, 0, 0], "no arm present"),
]
GROUPS = (3, 5)


def rows(arms):
    """-> scores [R, arms] float32, mask [R, arms] bool"""
    named = {3: NAMED, 5: NAMED5}[arms]
    scores, mask = [r[0] for r in named], [r[1] for r in named]
    if arms == 3:
        for s in itertools.product((-INF, 1.0, INF, NAN), repeat=3):
            for m in itertools.product((0, 1), repeat=3):
                scores.append(list(s))
                mask.append(list(m))
    return torch.tensor(scores, dtype=torch.float32), torch.tensor(mask, dtype=torch.bool)


def generate():
    import warnings

    _install()
    from reagent.training.cb.utils import get_model_actions

    arrays = {}
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")  # (torch.masked is a prototype and says so)
        for arms in GROUPS:
            scores, mask = rows(arms)
            # row by row as well as in one call: the reference's answer for a row must not depend on its neighbours
            masked = get_model_actions(scores.clone(), mask.clone())
            plain = get_model_actions(scores.clone())
            for r in range(scores.shape[0]):
                one = get_model_actions(scores[r:r + 1].clone(), mask[r:r + 1].clone())
                assert torch.equal(one, masked[r:r + 1]), (arms, r)
            assert masked.shape == plain.shape == (scores.shape[0], 1)
            arrays[f"a{arms}_scores"] = _np(scores)
            arrays[f"a{arms}_mask"] = _np(mask)
            arrays[f"a{arms}_actions_masked"] = _np(masked).astype(np.int64)
            arrays[f"a{arms}_actions_plain"] = _np(plain).astype(np.int64)
    return arrays


def main():
    check = "--check" in sys.argv[1:]
    os.makedirs(OUT, exist_ok=True)
    arrays = generate()
    path = os.path.join(OUT, NAME + ".npz")
    if check:
        with np.load(path) as old:
            same = sorted(old.files) == sorted(arrays) and all(
                old[k].dtype == arrays[k].dtype and old[k].shape == arrays[k].shape
                and np.array_equal(old[k], arrays[k], equal_nan=old[k].dtype.kind == "f") for k in arrays)
        print(NAME, "identical" if same else "DIFFERS")
        sys.exit(0 if same else 1)
    np.savez_compressed(path, **arrays)
    print("wrote", NAME, sum(a.nbytes for a in arrays.values()) // 1024, "KiB")


if __name__ == "__main__":
    main()
