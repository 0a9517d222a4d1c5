"""The self-collision case that the rows-kernel tests on both sides share (tests/test_gpu_terms.py, tests/test_oracle_rbd.py).  A plain module."""
from inria_wbc_amd import model as mdl
from inria_wbc_amd import structure

BATCH = 3                                              # states the parity test draws for this case
STATES = dict(seed=31_000, q_noise=0.3, v_noise=0.5, ref_noise=0.2)  # as tests/test_gpu_terms.py draws them for every tree case


def tree_65_pairs():
    """More self-collision pairs than a wave has lanes: five tasks of 13 avoided frames each on a fixed-base tree of 12 bodies,
    65 pairs over 18 distinct frames.  The kernel's pair loop takes 64 pairs per pass, so pair 64 (the last avoided frame of the
    last task) is the one pair of its SECOND pass, which fetches that pair's tables anew (the host caps frames, blocks and laws
    at 64, not pairs).  tests/test_oracle_rbd.py::test_pair_64_of_the_65_pair_case_is_active holds the case itself: 65 pairs,
    and the last one moves the oracle's row, so the comparison cannot pass with the second pass skipped."""
    m = mdl.random_tree(25, 12, False, nframe=18)
    stack = [dict(name="hand", type="se3", tracked="f17", kp=20.0, mask="111111"), dict(name="posture", type="posture", kp=10.0),
             dict(name="bounds", type="bounds")]
    for t in range(5):
        avoided = {"f%d" % ((t + 1 + k) % 18): 0.5 + 0.05 * k for k in range(13)}
        stack.append(dict(name="sc_%d" % t, type="self-collision", tracked="f%d" % t, radius=0.5, avoided=avoided, kp=50.0, kd=250.0,
                          margin=0.8, m=0.5))  # radii and margin of the size of the tree: most pairs are active
    st = structure._mk("tree_65_pairs", m.nv, m.na, [], [("hand", 6, 10.0), ("__posture__", "posture", 0.5)], None,
                       [("sc_%d" % t, 500.0) for t in range(5)], True, False, [(structure.INEQ_BOUNDS, 0)])
    return m, st, mdl.build_taskmap(m, st, stack, dt=2e-3)
