"""hipcc's resource report for the counterfactual-evaluation kernels (reagent_amd/csrc/bbb.hip): the expected kernels, no scratch
and no spilled registers."""
from kernel_remarks import kernel_resources

EXPECTED = ["bbb_fill_noise_kernel", "bbb_sample_kernel", "bbb_sample_finish_kernel", "bbb_grad_kernel", "bbb_elbo_rows_kernel",
            "bbb_elbo_finish_kernel", "bandit_rows_kernel", "bandit_finish_kernel"]


def test_kernels_have_no_scratch_and_no_spills(tmp_path):
    kernels = kernel_resources("bbb.hip", tmp_path)
    assert len(kernels) == len(EXPECTED), sorted(kernels)
    for want in EXPECTED:
        hits = [k for k in kernels if want in k]
        assert len(hits) == 1, (want, sorted(kernels))
        v = kernels[hits[0]]
        print(want, v)
        assert v.get("VGPRs Spill", 0) == 0 and v.get("SGPRs Spill", 0) == 0 and v["ScratchSize [bytes/lane]"] == 0, (want, v)
        assert v["VGPRs"] <= 64, (want, v)  # element-wise kernels: DESIGN.md section 3.20 states at most 38
