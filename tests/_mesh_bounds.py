"""The measured distance of the fp32 restatement of ``ga_mesh_point_distance`` (tests/_mesh_ops_ref.py: point_distance) from the float64
brute force (point_distance64), per mesh of the zoo over its query set (tests/test_mesh_ops_cpu.py: distance_queries):

    max |dist2 - dist2_64| / (dist2_64 + extent^2 * eps),   extent = max |vertex coordinate|,  eps = 2^-23

Produced by

    from tests import test_mesh_ops_cpu as t
    for name in t.zoo():
        print(name, t.measured_error(name))

(second figure: the same quantity between the float64 distances of the two chosen faces, where the fp32 and the float64 choice differ;
0.0 = they never differed).  Both sides are deterministic CPU code, so the asserted bound is the largest figure rounded up to two
significant digits and nothing more.  The gradient test of tests/test_point_mesh_gpu.py scales the same bound by the extent."""

MEASURED = {
    "icosphere0": (1.2739765184101848e-05, 0.0),
    "icosphere1": (1.1185600474108457e-05, 0.0),
    "icosphere2": (1.122694751599063e-05, 0.0),
    "icosphere3": (1.3084875812020441e-05, 0.0),
    "square": (5.251972103210957e-08, 0.0),
    "pair": (1.4368129110234366e-06, 0.0),
    "soup": (3.1449480731873996e-05, 0.0),
    "spliced": (3.1449480731873996e-05, 0.0),
    "ties": (3.3616977704306117e-06, 0.0),
}

DIST2_REL_BOUND = 3.2e-05   # max of MEASURED, rounded up to two significant digits
