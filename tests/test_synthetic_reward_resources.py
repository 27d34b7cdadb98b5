"""hipcc's resource report for the synthetic-reward kernels (reagent_amd/csrc/synthetic_reward.hip): the expected kernels, no
scratch and no spilled registers."""
from kernel_remarks import kernel_resources

EXPECTED = ["srw_ngram_kernel", "srw_head_kernel", "srw_finish_kernel", "srw_dh_kernel"]


def test_kernels_have_no_scratch_and_no_spills(tmp_path):
    kernels = kernel_resources("synthetic_reward.hip", tmp_path)
    assert len(kernels) == len(EXPECTED), sorted(kernels)
    for want in EXPECTED:
        hits = [k for k in kernels if want in k]
        assert len(hits) == 1, (want, sorted(kernels))
        v = kernels[hits[0]]
        print(want, v)
        assert v.get("VGPRs Spill", 0) == 0 and v.get("SGPRs Spill", 0) == 0 and v["ScratchSize [bytes/lane]"] == 0, (want, v)
        assert v["VGPRs"] <= 256, (want, v)
