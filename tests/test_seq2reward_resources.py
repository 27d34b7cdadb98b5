"""hipcc's resource report for the Seq2Reward kernels (reagent_amd/csrc/seq2reward.hip): the expected kernels, no scratch and
no spilled registers, and the fan-out step's LDS image within the CU's 160 KB at the widest hidden size."""
from kernel_remarks import kernel_resources

EXPECTED = ["s2r_fanout_kernel", "s2r_plan_max_kernel", "s2r_head_kernel", "s2r_finish_kernel", "s2r_step_ce_kernel"]


def test_kernels_have_no_scratch_and_no_spills(tmp_path):
    kernels = kernel_resources("seq2reward.hip", tmp_path)
    assert len(kernels) == len(EXPECTED), sorted(kernels)
    for want in EXPECTED:
        hits = [k for k in kernels if want in k]
        assert len(hits) == 1, (want, sorted(kernels))
        v = kernels[hits[0]]
        print(want, v)
        assert v.get("VGPRs Spill", 0) == 0 and v.get("SGPRs Spill", 0) == 0 and v["ScratchSize [bytes/lane]"] == 0, (want, v)
        assert v["VGPRs"] <= 256, (want, v)


def test_the_fanout_tile_fits_lds_at_the_widest_hidden_size():
    """the dynamic LDS the launch asks for at H = 256: one image of 32 x 257 floats (the parents' h), plus the exp table"""
    assert 32 * (256 + 1) * 4 + 128 <= 160 * 1024
