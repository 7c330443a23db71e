"""The cases of the batched transform queries under a uniform grid.  Nothing new is built here: the kernel cases of
tests/mesh_symmetry_cases.py (fp_mesh_transform_residuals) and tests/mesh_icp_cases.py (fp_mesh_icp_step) and the penetration cases of
tests/test_gpu_mesh_signed.py are paired with the six grids of tests/mesh_grid_cases.py.  Those cases already sit on the tiling
boundaries: Q of 1, 63 to 65, 255 to 257 and 1000, T of 1, 2, 3, 70 and 257, transforms with scale, NaN, inf and overflow, F = 0,
faces that are skipped or degenerate -- the smallest shapes at which the pair numbering n = t * Q + i, the finish strides and the
chunking can go wrong.

A (case, grid) is left out only when T * Q * ncells > CAP: a lane whose p' is far from the mesh (the NaN-free rows of the special
transforms, the scaled one) visits every cell of the grid, and the cap keeps such a walk by every lane within seconds.  Counted
here, that removes "tiny cells" from OMITTED_RESIDUALS of the residual cases and from OMITTED_ICP of the ICP cases and nothing
under the other five grids; the module asserts exactly that, so the cap can never quietly empty a grid kind."""
import functools

import numpy as np

import mesh_grid_cases as gcs
import mesh_icp_cases as ic
import mesh_symmetry_cases as sc

f32 = np.float32
CAP = 1 << 28
OMITTED_RESIDUALS, OMITTED_ICP = 8, 10                 # under "tiny cells", of 41 and of 44
PENETRATION_SIZES = ((1, 1), (2, 63), (70, 64), (257, 65), (1, 255), (2, 256), (70, 257), (257, 1000))   # test_penetration_equals_the_restatement's
# the pair cases the host test runs the model's walk on: every kind of transform and of face, and both finish strides
MODEL_CASES = (("residuals", "box special transforms"), ("residuals", "skipped and degenerate special transforms"),
               ("residuals", "soup F=40 Q=257 T=3"), ("icp", "skipped and degenerate special transforms"), ("icp", "three chunks T=5"),
               ("icp", "degenerate winning face"))


@functools.lru_cache(maxsize=None)
def grid(kind_of_case, name, kind):
    """the grid `kind` (mesh_grid_cases.GRIDS) over the mesh of a residual ("residuals") or ICP ("icp") kernel case"""
    c = case(kind_of_case, name)
    return gcs.grid_of(c["pos"], c["faces"], kind)


def case(kind_of_case, name):
    cases = sc.kernel_cases() if kind_of_case == "residuals" else ic.kernel_cases()
    return next(c for c in cases if c["name"] == name)


def admitted_by_size(T, Q, ncells):
    return T * Q * ncells <= CAP


def admitted(kind_of_case, c):
    """the grids a case runs under"""
    T, Q = len(c["tfs"]), len(c["points"])
    return tuple(k for k in gcs.GRIDS if admitted_by_size(T, Q, grid(kind_of_case, c["name"], k).ncells))


@functools.lru_cache(maxsize=None)
def omissions():
    """-> {"residuals": {grid kind: the names left out}, "icp": ...}"""
    out = {}
    for what, cases in (("residuals", sc.kernel_cases()), ("icp", ic.kernel_cases())):
        out[what] = {k: tuple(c["name"] for c in cases if k not in admitted(what, c)) for k in gcs.GRIDS}
    return out


def check_omissions():
    """no omission outside "tiny cells", and at most a quarter of the cases under it"""
    got = omissions()
    for what, cases in (("residuals", sc.kernel_cases()), ("icp", ic.kernel_cases())):
        for k in gcs.GRIDS:
            n = len(got[what][k])
            assert n == 0 or k == "tiny cells", (what, k, got[what][k])
            assert 4 * n <= len(cases), (what, k, n, len(cases))
    assert (len(got["residuals"]["tiny cells"]), len(got["icp"]["tiny cells"])) == (OMITTED_RESIDUALS, OMITTED_ICP)
    return got


check_omissions()


def penetration_case(dev, T, Q, seed=0):
    """test_gpu_mesh_signed._penetration_case with the grids it runs under -> (c, (vn, en), mesh, pts, tfs, {kind: mesh_grid_model.Grid})"""
    from test_gpu_mesh_signed import _penetration_case
    c, tables, mesh, pts, tfs = _penetration_case(dev, T, Q, seed)
    grids = {k: gcs.grid_of(c["pos"], c["faces"], k) for k in gcs.GRIDS}
    return c, tables, mesh, pts, tfs, {k: g for k, g in grids.items() if admitted_by_size(T, Q, g.ncells)}
