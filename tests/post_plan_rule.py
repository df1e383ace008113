"""Which kernel writes a dense Jacobian that the row launch did not write: the rule of csrc/post_plan.h and of the two assembly
launchers (kernels_post.hip), restated in Python integers so that a GPU test can say what it expects without asking the library.
tests/test_post_plan_cpu.py holds this restatement against the boundary the stand-alone check of the header prints."""

ASM_VPT, ASM_BLOCK = 4, 256          # 16-byte vectors per lane, lanes per workgroup

RAGGED, MISALIGNED, TOO_LARGE, INEXACT = "ragged", "misaligned", "too_large", "inexact"


def flat_refusal(mn, B, esz, ptr):
    """None when post_flat_kernel takes (B, mn) elements of esz bytes at address ptr, else the reason it does not."""
    nv = 16 // esz
    if mn % nv:
        return RAGGED
    if ptr % 16:
        return MISALIGNED
    if B * mn >= 1 << 32:
        return TOO_LARGE
    magic = -((-1 << 32) // mn)                      # ceil(2^32 / mn)
    err = magic * mn - (1 << 32)
    if magic >= 1 << 32 or err * (mn + ASM_BLOCK * ASM_VPT * nv) >= 1 << 32:
        return INEXACT
    return None


def first_inexact(esz, top):
    """Smallest mn <= top that the error bound of the reciprocal refuses (a whole number of vectors, aligned, B = 1)."""
    nv = 16 // esz
    return next((mn for mn in range(nv, top + 1, nv) if flat_refusal(mn, 1, esz, 0) == INEXACT), None)


def assembly_writer(mn, B, esz, ptr, resident, objective):
    """Name (CallbackEngine.last_dense_writer) of the assembly launch behind a row launch that left the dense matrix to it.
    resident: the pointer is a registered resident buffer covering B; objective: f or grad go out with the same launch (they
    do not when tracking data are bound: the binding's own kernel follows)."""
    if resident:
        return "post_scatter_kernel"
    if flat_refusal(mn, B, esz, ptr) is None:
        return "post_flat_kernel"
    return "post_kernel" if objective else "assemble_dense_kernel"
