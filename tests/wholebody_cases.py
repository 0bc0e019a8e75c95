"""Poses for the whole-body tests (test_wholebody_host.py, test_gpu_wholebody.py): the persons of
four golden fixtures and synthetic persons chosen to take every branch of ``wholebody.body_rois_np``."""
import numpy as np

from conftest import load_golden, pkg_module

FIXTURES = ("six_people", "portrait_four", "one_person", "twenty_720p")
NOSE, R_ELBOW, R_HAND, L_ELBOW, L_HAND = 0, 3, 4, 6, 7
BASE_LIMBS = (14, 3, 0, 13, 9)


def fixture_poses():
    """(31, 18, 3): the persons of the four fixtures, in FIXTURES order."""
    return np.concatenate([load_golden(name)["poses"].reshape(-1, 18, 3) for name in FIXTURES])


def limbs():
    return [(int(a), int(b)) for a, b in pkg_module("constants").params["limbs_point"]]


def clustered(rng, zero_limbs=(), lo=40.0, hi=400.0):
    """A person with every joint found whose limbs ``zero_limbs`` (and whatever they close) have
    length 0: the joints a zero limb joins share one point, every other point is drawn apart."""
    parent = list(range(18))

    def root(j):
        while parent[j] != j:
            j = parent[j]
        return j

    L = limbs()
    for i in zero_limbs:
        a, b = L[i]
        parent[root(a)] = root(b)
    points = {}
    pose = np.zeros((18, 3))
    for j in range(18):
        r = root(j)
        if r not in points:
            points[r] = rng.uniform(lo, hi, 2)
        pose[j] = (points[r][0], points[r][1], 2.0)
    return pose


def found_limbs(pose):
    return sum(1 for a, b in limbs() if not (pose[a][0] == pose[b][0] and pose[a][1] == pose[b][1]))


def synthetic():
    """-> (poses (n, 18, 3), names).  Every case of the issue's list; the names say which.

    The unit's sum never has more than 14 terms: it takes all 19 divisors only when the five base
    limbs have length 0.  So the fallback persons have exactly 7, 8, 9 and 14 found limbs (both sides
    of the 8-term seam of the pairwise sum, and the longest sum there is), and the persons with
    exactly 16, 17 and 19 found limbs take the base branch; ``pairwise_sum`` itself is held to
    ``np.sum`` for every n <= 19 on the host."""
    rng = np.random.default_rng(5)
    cases = []
    base0 = list(BASE_LIMBS)
    for want, extra in ((14, []), (9, [2, 5, 8, 12, 1]), (8, [2, 5, 8, 12, 1, 4]), (7, [2, 5, 8, 12, 1, 4, 7])):
        p = clustered(rng, base0 + extra)
        assert found_limbs(p) == want, (want, found_limbs(p))
        cases.append(("fallback_%d_found" % want, p))
    for want, zero in ((19, []), (17, [2, 5]), (16, [2, 5, 8])):
        p = clustered(rng, zero)
        assert found_limbs(p) == want, (want, found_limbs(p))
        cases.append(("base_%d_found" % want, p))
    p = clustered(rng)
    p[L_ELBOW] = 0.0  # absent: at (0, 0), as a pose row holds it
    cases.append(("left_elbow_absent_no_shift", p))
    p = clustered(rng)
    p[R_HAND, :2] = p[R_ELBOW, :2]
    cases.append(("right_hand_on_its_elbow", p))
    p = clustered(rng, lo=100.0, hi=100.01)
    cases.append(("unit_below_one_pixel_state_2", p))
    p = clustered(rng)
    p[L_HAND, 0] = np.nan
    cases.append(("nan_left_hand_state_2", p))
    p = clustered(rng)
    p[NOSE, 1] = np.nan
    cases.append(("nan_nose_state_2", p))
    p = clustered(rng)
    p[R_HAND, 0] = 1e12
    cases.append(("1e12_right_hand_state_2", p))
    p = clustered(rng)
    p[NOSE, 0] = np.inf
    cases.append(("inf_nose_unit_not_finite", p))
    p = clustered(rng, lo=-90.0, hi=-3.0)
    cases.append(("negative_coordinates_trunc_is_not_floor", p))
    p = clustered(rng, lo=-30.0, hi=30.0)
    cases.append(("coordinates_across_zero", p))
    p = clustered(rng, list(range(19)))
    cases.append(("one_point_no_limb_unit_nan", p))
    p = clustered(rng)
    p[[NOSE, L_HAND, R_HAND]] = 0.0
    cases.append(("no_nose_no_hands", p))
    p = np.zeros((18, 3))
    p[[1, 2, 5]] = [[120.5, 80.25, 2.0], [100.75, 82.5, 2.0], [141.0, 81.125, 2.0]]
    cases.append(("three_joints", p))
    return np.stack([c[1] for c in cases]), [c[0] for c in cases]
