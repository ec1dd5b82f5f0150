"""Which k_block_op instantiation runs for an operator: a Python restatement of the three flag expressions and of the
launch cascade as fusmi.hip held them before csrc/block_variant.hpp existed (op_build: `pk`, `gcs`; op_setup_device:
`mfma`, `diag`; launch_block_op: the cascade).  Written from that file, not from the header, so that the two can
disagree.  tests/test_block_variant_host.py compares the header with it over the whole input space,
tests/test_gpu_block_variant.py compares what a live operator reports."""

STREAM, AFFINE, TRILINEAR, DIAG = 0, 1, 2, 3   # GEOM_* (and the geometry mode: 0, 1, 2)
STIFFNESS, MASS = 0, 1
STAGE_NONE = -1
STAGES = (-1, 0, 1, 3, 4, 5, 6, 7)


def mfma_default(P, f64, affine):
    return False


def build_flags(P, nbytes, tdim, pred, ortho, c_deterministic, o_mfma, o_pack32, o_diag_metric, flip=None):
    """op_build: (pk, gcs) from the host-predicted mode.  `ortho` is op->ortho_mesh."""
    affine_mesh, trilinear_mesh = pred == AFFINE, pred == TRILINEAR
    diag_mesh = bool(ortho and o_diag_metric and P <= 7 and not (o_mfma == 1) and not (o_pack32 == 1))
    auto = P == 5 or (P == 6 and affine_mesh)
    if flip == "pk_auto_p6":   # negative control: auto packs degree 6 on trilinear cells too
        auto = P == 5 or P == 6
    pk = bool(nbytes == 4 and tdim == 3 and 5 <= P <= 7 and (affine_mesh or trilinear_mesh)
              and not c_deterministic and o_mfma != 1
              and (o_pack32 == 1 or (o_pack32 < 0 and not diag_mesh and auto)))
    gcs = 7 if affine_mesh else (21 if trilinear_mesh else 0)
    return pk, gcs


def setup_flags(P, nbytes, conf, ortho, o_deterministic, o_mfma, o_diag_metric, pk):
    """op_setup_device: (mfma, diag, gcs) from the device-confirmed mode and the layout's pk."""
    affine, trilinear = conf == AFFINE, conf == TRILINEAR
    mfma = bool(P in (6, 7) and (affine or trilinear) and not o_deterministic
                and (o_mfma == 1 or (o_mfma < 0 and mfma_default(P, nbytes == 8, affine))))
    diag = bool(affine and ortho and o_diag_metric and P <= 7 and not mfma and not pk)
    return mfma, diag, 7 if affine else (21 if trilinear else 0)


def cascade(P, nbytes, tdim, conf, deterministic, mfma, pk, diag, OP, STAGE):
    """launch_block_op: (GEOM, TD, ATOMIC, MF, PK) of the launch."""
    affine, trilinear = conf == AFFINE, conf == TRILINEAR
    atomic = 0 if deterministic else 1
    if P >= 8:
        if tdim == 2:
            return (STREAM, 2, atomic, 0, 0)
        if not (affine or trilinear):
            return (STREAM, 3, atomic, 0, 0)
        return (AFFINE if affine else TRILINEAR, 3, atomic, 0, 0)
    if tdim == 2:
        return (STREAM, 2, atomic, 0, 0)
    if P in (6, 7) and OP == STIFFNESS and (STAGE == STAGE_NONE or STAGE >= 3):
        if mfma and not deterministic and tdim == 3 and (affine or trilinear):
            return (AFFINE if affine else TRILINEAR, 3, 1, 1, 0)
    if nbytes == 4 and 5 <= P <= 7 and OP == STIFFNESS:
        if pk and not mfma and not deterministic and tdim == 3 and (affine or trilinear):
            return (AFFINE if affine else TRILINEAR, 3, 1, 0, 1)
    if OP == STIFFNESS and P <= 7:
        if affine and diag:
            return (DIAG, 3, atomic, 0, 0)
    if affine:
        return (AFFINE, 3, atomic, 0, 0)
    if trilinear:
        return (TRILINEAR, 3, atomic, 0, 0)
    return (STREAM, 3, atomic, 0, 0)


def instantiated(P, nbytes, OP, STAGE, v):
    """Is k_block_op<T, P, OP, ATOMIC, STAGE, NF, GEOM, TD, MF, PK> one of the kernels that cascade could launch?"""
    geom, td, atomic, mf, pk = v
    if td == 2:
        return geom == STREAM and not mf and not pk
    if mf:
        return P in (6, 7) and OP == STIFFNESS and (STAGE == STAGE_NONE or STAGE >= 3) and atomic == 1 and not pk and geom in (AFFINE, TRILINEAR)
    if pk:
        return nbytes == 4 and 5 <= P <= 7 and OP == STIFFNESS and atomic == 1 and geom in (AFFINE, TRILINEAR)
    if geom == DIAG:
        return OP == STIFFNESS and P <= 7
    return geom in (STREAM, AFFINE, TRILINEAR)


def decide(P, nbytes, tdim, pred, conf, ortho, deterministic, o_mfma, o_pack32, o_diag_metric, flip=None):
    """The whole decision for one operator: dict with pk, gcs_pred, mfma, diag, gcs and variant(OP, STAGE)."""
    pk, gcs_pred = build_flags(P, nbytes, tdim, pred, ortho, deterministic, o_mfma, o_pack32, o_diag_metric, flip)
    mfma, diag, gcs = setup_flags(P, nbytes, conf, ortho, deterministic, o_mfma, o_diag_metric, pk)
    return dict(pk=pk, gcs_pred=gcs_pred, mfma=mfma, diag=diag, gcs=gcs,
                variant=lambda OP, STAGE: cascade(P, nbytes, tdim, conf, deterministic, mfma, pk, diag, OP, STAGE))


def introspection(P, nbytes, tdim, mode, ortho, deterministic, o_mfma=-1, o_pack32=-1, o_diag_metric=1):
    """What fus_op_geometry_mode / uses_mfma / uses_pack32 / uses_diag_metric / uses_mfma4 answered for such an operator."""
    d = decide(P, nbytes, tdim, mode, mode, ortho, deterministic, o_mfma, o_pack32, o_diag_metric)
    return dict(geometry_mode=mode, uses_mfma=int(d["mfma"]), uses_pack32=int(d["pk"] and not d["mfma"]),
                uses_diag_metric=int(d["diag"]),
                uses_mfma4=int(P == 7 and nbytes == 8 and tdim == 3 and mode == TRILINEAR and not d["mfma"]))
