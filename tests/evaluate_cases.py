"""What tests/test_policy_evaluate.py (CPU guard) and tests/test_gpu_policy_evaluate.py share: the capture flags of an
oracle run and the conditions a closed-loop case (tests/policy_cases.py) must meet for a summary-record comparison to
mean something.  Needs numpy and the package's `policy` module only."""
import numpy as np

from underwater_swimmer_rl_amd.policy import evaluation_views

CUT = 100       # the split of "split equals whole": 100 steps, then the rest with SALP_EVAL_ACCUMULATE


def captures_from_info(info, terminated, truncated, start_count=0, autoreset=True):
    """bool [H, n]: the env captured a food in that step.  `info[..., 0]` is food_collected of the step's own episode
    (before a same-step autoreset), so a capture is an increase over the step before, the counter starting again from zero
    behind a finished step (autoreset) and from `start_count` at step 0."""
    fc = np.asarray(info)[..., 0].astype(np.int64)
    done = (np.asarray(terminated).astype(bool) | np.asarray(truncated).astype(bool))
    prev = np.empty_like(fc)
    prev[0] = start_count
    prev[1:] = np.where(done[:-1], 0, fc[:-1]) if autoreset else fc[:-1]
    d = fc - prev
    assert ((d == 0) | (d == 1)).all(), "food_collected moves by at most one per step"
    return d == 1


def assert_not_vacuous(name, record, cut=CUT):
    """Every case must end episodes both ways, more than once per env somewhere, capture food, and have first episode ends
    on both sides of the cut."""
    v = evaluation_views(record)
    n_term, n_trunc = int((v["first_end"] == 1).sum()), int((v["first_end"] == 2).sum())
    n_twice, food = int((v["episodes"] >= 2).sum()), int(v["food"].sum())
    finished = v["first_end"] != 0
    before, after = int((finished & (v["first_length"] <= cut)).sum()), int((finished & (v["first_length"] > cut)).sum())
    figures = dict(first_end_terminated=n_term, first_end_truncated=n_trunc, episodes_twice=n_twice, food=food,
                   first_end_before_cut=before, first_end_after_cut=after)
    print(f"{name}: {figures}")
    assert n_term >= 1 and n_trunc >= 1 and n_twice >= 1 and food >= 1 and before >= 1 and after >= 1, f"{name}: {figures}"
    return figures
