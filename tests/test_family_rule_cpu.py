"""The kernel-family rule (stereo_amd/csrc/trws_family.h, stereo_trws_family_rule) against the booleans it replaced.

Until the rule was written down once, a plan kept five booleans -- fast, fast2, wide_allowed and large from its
creation, wide from every upload -- and `stereo_trws_plan_path` read them in the order large, wide, fast2, fast.  That
logic is restated here literally, with the refusals in the order a caller met them (creation first, then the
upload), and compared with the rule over the full product of its facts.  Host only: no device is touched."""
import ctypes as C
import itertools

import pytest

EXACT, MINPLUS = 0, 1

K_RANGE = ("stereo_trws: K must be in [1, 512] (up to 4096 with one strictly ascending positions vector shared by "
           "every edge)")
STRIP_GRAPH = ("stereo_trws: row strips need a graph the pipelined kernels take (<= 8 edges per node, <= 4 "
               "dependencies in other runs, a chain schedule that provably terminates)")
STRIP_LABELS = ("stereo_trws: row strips need a graph and label count the pipelined kernels take (<= 8 edges per "
                "node; K <= 64, or K <= 128 with per-edge positions, or K <= 256 with shared ascending positions)")
STRIP_INPUTS = ("stereo_trws: row strips with these inputs would need the generic kernel, which has no strip support "
                "(K > 128 or the MINPLUS mode need shared strictly ascending positions)")

KS = (1, 2, 63, 64, 65, 127, 128, 129, 255, 256, 257, 511, 512, 513, 1024, 4096, 4097)
PER_EDGE, SHARED, SHARED_ASCENDING = 0, 1, 2


def the_old_booleans(kernel, K, mode, fast_ok, fast_on, strips, positions, lam):
    """(path, None) or (0, error text): what plan creation followed by an upload gave."""
    exact = mode == EXACT
    # stereo_trws_plan_create
    if K < 1 or K > 4096:
        return 0, K_RANGE
    if strips and not fast_ok:
        return 0, STRIP_GRAPH
    fast = fast_ok and K <= 64 and exact
    fast2 = fast_ok and 64 < K <= 128 and exact
    wide_allowed = fast_ok and (kernel == 1 or exact) and 64 < K <= 256
    fast, fast2, wide_allowed = fast and fast_on, fast2 and fast_on, wide_allowed and fast_on
    large = K > 512
    if strips and not (fast or wide_allowed or fast2):
        return 0, STRIP_LABELS
    # stereo_trws_plan_upload / finish_inputs
    shared = positions != PER_EDGE
    ascending = positions == SHARED_ASCENDING
    if large and not (shared and ascending):
        return 0, K_RANGE
    wide = wide_allowed and shared and ascending and lam >= 0
    if strips and not (fast or fast2 or wide):
        return 0, STRIP_INPUTS
    return (5 if large else 3 if wide else 4 if fast2 else 2 if fast else 1), None


@pytest.fixture(scope="module")
def rule():
    from stereo_amd import _lib
    fn = _lib.lib().stereo_trws_family_rule
    fn.restype = C.c_int
    fn.argtypes = [C.c_int] * 7 + [C.c_double, C.c_char_p, C.c_size_t]

    def call(kernel, K, mode, fast_ok, fast_on, strips, positions, lam):
        err = C.create_string_buffer(1024)
        family = fn(kernel, K, mode, int(fast_ok), int(fast_on), int(strips), positions, float(lam), err, len(err))
        return family, (err.value.decode() if family == 0 else None)
    return call


@pytest.mark.parametrize("K", KS)
def test_the_rule_is_the_old_booleans(rule, K):
    from stereo_amd.trws import MESSAGES_EXACT, MESSAGES_MINPLUS
    assert (MESSAGES_EXACT, MESSAGES_MINPLUS) == (EXACT, MINPLUS)
    n = 0
    for kernel, mode, fast_ok, fast_on, strips, positions, lam in itertools.product(
            (1, 2), (EXACT, MINPLUS), (False, True), (True, False), (False, True),
            (PER_EDGE, SHARED, SHARED_ASCENDING), (-1.0, 0.0, 8.0)):
        facts = (kernel, K, mode, fast_ok, fast_on, strips, positions, lam)
        assert rule(*facts) == the_old_booleans(*facts), facts
        n += 1
    assert n == 2 * 2 * 2 * 2 * 2 * 3 * 3


def test_every_family_and_every_refusal_occurs(rule):
    seen = set()
    for K in KS:
        for rest in itertools.product((1, 2), (EXACT, MINPLUS), (False, True), (True, False), (False, True),
                                      (PER_EDGE, SHARED, SHARED_ASCENDING), (-1.0, 0.0, 8.0)):
            family, err = rule(rest[0], K, *rest[1:])
            seen.add(family or err)
    assert seen == {1, 2, 3, 4, 5, K_RANGE, STRIP_GRAPH, STRIP_LABELS, STRIP_INPUTS}


def test_a_plan_without_inputs_is_never_refused_for_them(rule):
    """positions = -1 (what a plan reports before its first upload): the family of per-edge positions, the large family
    above 512 labels, and no refusal that an upload could still avoid."""
    for K in KS:
        for kernel, mode, fast_ok, fast_on, strips in itertools.product((1, 2), (EXACT, MINPLUS), (False, True),
                                                                         (True, False), (False, True)):
            old, err = the_old_booleans(kernel, K, mode, fast_ok, fast_on, strips, PER_EDGE, 0.0)
            if err in (K_RANGE, STRIP_INPUTS) and 1 <= K <= 4096:
                old, err = (5 if K > 512 else 1), None
            assert rule(kernel, K, mode, fast_ok, fast_on, strips, -1, 0.0) == (old, err)
