"""The flat form of a cloud (pwn_hip_cloud_export / pwn_hip_cloud_import; CloudFlatHeader in pwn_hip_capi.hip) read and written in numpy, and
clouds of the CONVERTER'S form made from the injected arrays of tests/align_clouds.py: no Omega_n planes but a curvature threshold and two class
matrices (CloudDev::OmN == nullptr: the class-table path of the fused pass, load_omegas' class branch, the class expansion of the download and of
k_expand_omega_n), and a stored index image with its key (the aligner's projection shortcuts).  A helper module of the tests; nothing here needs
a GPU at import.

Layout: a 256-byte header, then sections at multiples of 256 bytes: P3 (12 n bytes), Nc (16 n: normal, curvature), om_planes Omega_p planes of
12 n bytes each (3 for exact9, 2 for sym6), optionally 3 Omega_n planes, then the index image (4 bytes per pixel).
"""
from __future__ import annotations

import numpy as np

import align_clouds as A

F32 = np.float32
MAGIC = 0x464E5750                                  # "PWNF"
HEADER = np.dtype([("magic", "<u4"), ("version", "<u4"), ("n", "<i4"), ("omSym", "<i4"), ("hasOmN", "<i4"), ("idxValid", "<i4"), ("idxRows", "<i4"),
                   ("idxCols", "<i4"), ("clsThr", "<f4"), ("idxMinD", "<f4"), ("idxMaxD", "<f4"), ("omN", "<f4", (2, 9)), ("idxK", "<f4", (9,)),
                   ("offP3", "<u8"), ("offNc", "<u8"), ("offOm", "<u8"), ("offOmN", "<u8"), ("offIdx", "<u8"), ("total", "<u8"), ("pad", "u1", (56,))])
assert HEADER.itemsize == 256
OFFSETS = ("offP3", "offNc", "offOm", "offOmN", "offIdx", "total")
SHIPPED_TABLE = np.stack([np.eye(3, dtype=F32) * F32(100.0), np.eye(3, dtype=F32)])      # NormalInformationMatrixCalculator: flat, non-flat


def up256(b):
    return (int(b) + 255) & ~255


def om_planes(om_sym):
    return 2 if om_sym else 3


def layout(n, om_sym, has_omn, pixels):
    """the six offsets of a flat cloud of n points (flat_layout)"""
    o = HEADER.itemsize
    out = {}
    out["offP3"] = o; o += up256(n * 12)
    out["offNc"] = o; o += up256(n * 16)
    out["offOm"] = o; o += om_planes(om_sym) * up256(n * 12)
    out["offOmN"] = o; o += 3 * up256(n * 12) if has_omn else 0
    out["offIdx"] = o; o += up256(pixels * 4)
    out["total"] = o
    return out


def parse(buf):
    """flat bytes -> dict: n, om_sym, cls_thr, omN [2, 9] (row-major 3x3 each: flat, non-flat), idx_K [9], idx_min_d, idx_max_d, P3 [n, 3],
    Nc [n, 4], Om [planes, n, 3], OmN [3, n, 3] or None, index [rows, cols] int32 or None.  The header's offsets are checked against the layout."""
    b = np.ascontiguousarray(buf, np.uint8).tobytes()
    h = np.frombuffer(b, HEADER, 1)[0]
    assert int(h["magic"]) == MAGIC and int(h["version"]) == 1, "not a flat cloud"
    n, sym, has_omn = int(h["n"]), int(h["omSym"]), int(h["hasOmN"]) != 0
    idx = int(h["idxValid"]) != 0 and int(h["idxRows"]) > 0 and int(h["idxCols"]) > 0
    rows, cols = (int(h["idxRows"]), int(h["idxCols"])) if idx else (0, 0)
    want = layout(n, sym, has_omn, rows * cols)
    assert all(int(h[k]) == want[k] for k in OFFSETS), ({k: int(h[k]) for k in OFFSETS}, want)
    assert len(b) >= want["total"]
    planes = lambda off, k: np.stack([np.frombuffer(b, F32, 3 * n, off + r * up256(n * 12)).reshape(n, 3) for r in range(k)]) if n else np.zeros((k, 0, 3), F32)
    return dict(n=n, om_sym=sym, cls_thr=F32(h["clsThr"]), omN=np.array(h["omN"], F32), idx_K=np.array(h["idxK"], F32), idx_min_d=F32(h["idxMinD"]),
                idx_max_d=F32(h["idxMaxD"]), P3=np.frombuffer(b, F32, 3 * n, want["offP3"]).reshape(n, 3).copy(),
                Nc=np.frombuffer(b, F32, 4 * n, want["offNc"]).reshape(n, 4).copy(), Om=planes(want["offOm"], om_planes(sym)).copy(),
                OmN=planes(want["offOmN"], 3).copy() if has_omn else None,
                index=np.frombuffer(b, np.int32, rows * cols, want["offIdx"]).reshape(rows, cols).copy() if idx else None)


def write(x):
    """the inverse of parse: a uint8 array of exactly layout(...)["total"] bytes, gaps zero"""
    n, sym = int(x["n"]), int(x["om_sym"])
    idx = x["index"] is not None
    rows, cols = x["index"].shape if idx else (0, 0)
    lay = layout(n, sym, x["OmN"] is not None, rows * cols)
    h = np.zeros(1, HEADER)
    h["magic"], h["version"], h["n"], h["omSym"], h["hasOmN"] = MAGIC, 1, n, sym, 0 if x["OmN"] is None else 1
    h["idxValid"], h["idxRows"], h["idxCols"] = (1 if idx else 0), rows, cols
    h["clsThr"], h["idxMinD"], h["idxMaxD"] = x["cls_thr"], x["idx_min_d"], x["idx_max_d"]
    h["omN"] = np.asarray(x["omN"], F32).reshape(2, 9); h["idxK"] = np.asarray(x["idx_K"], F32).reshape(9)
    for k in OFFSETS:
        h[k] = lay[k]
    out = np.zeros(lay["total"], np.uint8)
    def put(off, a, dt=F32):
        raw = np.ascontiguousarray(a, dt).view(np.uint8).reshape(-1)
        out[off:off + raw.size] = raw
    put(0, h, HEADER)
    assert x["P3"].shape == (n, 3) and x["Nc"].shape == (n, 4) and x["Om"].shape == (om_planes(sym), n, 3)
    put(lay["offP3"], x["P3"]); put(lay["offNc"], x["Nc"])
    for r in range(om_planes(sym)):
        put(lay["offOm"] + r * up256(n * 12), x["Om"][r])
    if x["OmN"] is not None:
        assert x["OmN"].shape == (3, n, 3)
        for r in range(3):
            put(lay["offOmN"] + r * up256(n * 12), x["OmN"][r])
    if idx:
        put(lay["offIdx"], x["index"], np.int32)
    return out


def same(a, b):
    """two parsed flat clouds hold the same bits"""
    bits = lambda v: np.ascontiguousarray(v).view(np.uint8).tobytes()
    for k in a:
        if (a[k] is None) != (b[k] is None):
            return False
        if a[k] is not None and (np.shape(a[k]) != np.shape(b[k]) or bits(np.asarray(a[k])) != bits(np.asarray(b[k]))):
            return False
    return set(a) == set(b)


def flat_bytes(cloud):
    """the cloud as pwn_hip_cloud_export writes it: every array, the stored index image and what it was made with"""
    buf = np.zeros(cloud.flatSize(), np.uint8)
    assert cloud.exportFlat(buf) == buf.size
    return buf


def stored_index(cloud):
    """(rows, cols, camera matrix, index image) the cloud keeps for the aligner's projection shortcuts, read from its flat form"""
    x = parse(flat_bytes(cloud))
    assert x["index"] is not None
    return x["index"].shape[0], x["index"].shape[1], x["idx_K"], x["index"]


# ---------------------------------------------------------------------------------------------------------------- the class rule
def rotated_table():
    """R diag(100, 50, 25) R^t and R' diag(1, 2, 3) R'^t, every entry evaluated and rounded in fp32 on its own (as the converter evaluates
    U diag U^t, informationmatrixcalculator.cpp:26-30): the mirror entries differ in their last bits"""
    R = A.axis_angle((1, 2, 3), 40.0)[:3, :3]; R2 = A.axis_angle((-2, 1, 0.5), 75.0)[:3, :3]
    return np.stack([A.omega_converter(R[None], np.array([[100.0, 50.0, 25.0]]))[0], A.omega_converter(R2[None], np.array([[1.0, 2.0, 3.0]]))[0]]).astype(F32)


TABLES = {"shipped": SHIPPED_TABLE, "rotated": rotated_table()}


def classes_by_rule(arrays, cls_thr, less=np.less, curvature=None):
    """NormalInformationMatrixCalculator::compute (informationmatrixcalculator.cpp:46-57) per point: 0 where the fp32 squared norm of the normal
    is 0, else 1 (flat) where curvature < cls_thr, else 2.  `less` and `curvature` are for the wrong rules the CPU test tells apart."""
    nrm = arrays["normals"].astype(F32)
    with np.errstate(under="ignore"):
        sq = A.dot3(nrm[:, :3], nrm[:, :3])
    cv = arrays["curvature"] if curvature is None else curvature
    return np.where(sq == 0, 0, np.where(less(cv.astype(F32), F32(cls_thr)), 1, 2)).astype(np.int32)


def omega_n_of_classes(cls, table):
    """[n, 16] column-major 4x4 normal information matrices of the classes (0: the zero matrix)"""
    t = np.concatenate([np.zeros((1, 3, 3), F32), np.asarray(table, F32).reshape(2, 3, 3)])
    M = np.zeros((len(cls), 4, 4), F32); M[:, :3, :3] = t[cls]
    return M.transpose(0, 2, 1).reshape(len(cls), 16).copy()


def omega_n_by_rule(arrays, table, cls_thr):
    return omega_n_of_classes(classes_by_rule(arrays, cls_thr), table)


def oracle_arrays(case, storage, table, cls_thr):
    """(reference, current) arrays for the oracle: the case's, with Omega_n replaced by the class rule"""
    out = []
    for a in (case.ref, case.cur):
        a = dict(A.arrays_for(a, storage))
        a["omega_n"] = omega_n_by_rule(a, table, cls_thr)
        out.append(a)
    return out


# ---------------------------------------------------------------------------------------------------------------- clouds of the converter's form
_keys = {}


def index_key(ctx, case):
    """(idxK, idxMinD, idxMaxD) in the library's own words: the header of a cloud DepthImageConverter.compute made with the case's camera and range"""
    k = (id(ctx), case.rows, case.cols, case.K, case.params["min_distance"], case.params["max_distance"])
    if k not in _keys:
        from g2o_frontend_amd import api
        proj = A.gpu_aligner(ctx, case).projector()
        conv = api.DepthImageConverterIntegralImage(proj, api.StatsCalculatorIntegralImage(), api.PointInformationMatrixCalculator(), api.NormalInformationMatrixCalculator())
        c = api.Cloud(ctx, case.rows * case.cols)
        conv.compute(c, np.full((case.rows, case.cols), 2.0, F32), images=False)
        x = parse(flat_bytes(c))
        assert x["index"] is not None and x["index"].shape == (case.rows, case.cols) and x["OmN"] is None
        _keys[k] = (x["idx_K"], x["idx_min_d"], x["idx_max_d"])
    return _keys[k]


def converter_form(ctx, case, side, table, cls_thr, with_index):
    """the case's `side` ("ref" / "cur") cloud as the converter would have left it: uploaded, exported, its Omega_n section dropped for the class
    table and the threshold, the case's index image stored under the library's own key, imported into a fresh cloud of the same storage"""
    from g2o_frontend_amd import api
    a = getattr(case, side)
    n = len(a["points"])
    up = api.Cloud(ctx, max(1, n))
    up.upload(a["points"], a["normals"], a["curvature"], a["omega_p"], a["omega_n"])
    x = parse(flat_bytes(up))
    assert x["n"] == n and x["OmN"] is not None
    x["OmN"] = None
    x["cls_thr"] = F32(cls_thr); x["omN"] = np.asarray(table, F32).reshape(2, 9)
    if with_index:
        x["idx_K"], x["idx_min_d"], x["idx_max_d"] = index_key(ctx, case)
        x["index"] = np.ascontiguousarray(case.cur_index if side == "cur" else case.ref_index, np.int32)
        assert x["index"].max(initial=-1) < n
    else:
        x["index"] = None
    out = api.Cloud(ctx, max(1, n))
    out.importFlat(write(x))
    assert out.size() == n and out.omega_storage() == up.omega_storage()
    return out
