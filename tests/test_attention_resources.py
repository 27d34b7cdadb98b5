"""hipcc's resource report for the attention kernels (reagent_amd/csrc/attention.hip): the expected kernels, no scratch and no
spilled registers, and the widest pair's LDS image within the CU's 160 KB."""
from kernel_remarks import kernel_resources

EXPECTED = ["attn_forward_kernel", "attn_backward_kernel", "residual_join_kernel", "residual_join_backward_kernel"]


def test_kernels_have_no_scratch_and_no_spills(tmp_path):
    kernels = kernel_resources("attention.hip", tmp_path)
    assert len(kernels) == len(EXPECTED), sorted(kernels)
    for want in EXPECTED:
        hits = [k for k in kernels if want + "E" in k]  # (the mangled name: ...<name>ENS_...)
        assert len(hits) == 1, (want, sorted(kernels))
        v = kernels[hits[0]]
        print(want, v)
        assert v.get("VGPRs Spill", 0) == 0 and v.get("SGPRs Spill", 0) == 0 and v["ScratchSize [bytes/lane]"] == 0, (want, v)
        assert v["VGPRs"] <= 256, (want, v)


def test_the_widest_pair_fits_lds():
    """floats of dynamic LDS a wave asks for at T = 64, hd = 128 (a workgroup is then one wave), plus the forward's exp table.
    Forward: a round's probabilities (64 doubles), q and v [T, hd], k [T, hd | 1]; backward: ds [T, T] in double, dctx (then k)
    [T, hd], v (then q) [T, hd | 1], p [T, T]"""
    T, hd = 64, 128
    forward = 128 + 2 * T * hd + T * (hd | 1)
    backward = 2 * T * T + T * hd + T * (hd | 1) + T * T
    assert 4 * forward + 128 <= 160 * 1024 and 4 * backward <= 160 * 1024
