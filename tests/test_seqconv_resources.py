"""hipcc's resource report for the sequence-convolution kernels (reagent_amd/csrc/seqconv.hip): the expected kernels, no scratch
and no spilled registers, and the largest LDS request (the window kernels' 32 KB image) within the CU's 160 KB."""
from kernel_remarks import kernel_resources

# kernel -> the VGPRs recorded in profiles/NOTES_r32.md and DESIGN.md 3.23 (a ceiling: more is a regression to look at)
EXPECTED = {"seqconv_forward_kernel": 75, "seqconv_dgrad_kernel": 75, "seqconv_wgrad_kernel": 61, "seqconv_wgrad_finish_kernel": 18,
            "ngram_window_kernel": 37, "ngram_window_backward_kernel": 17}


def test_kernels_have_no_scratch_no_spills_and_fit_lds(tmp_path):
    kernels = kernel_resources("seqconv.hip", tmp_path)
    assert len(kernels) == len(EXPECTED), sorted(kernels)
    for want, vgprs in EXPECTED.items():
        hits = [k for k in kernels if want + "E" in k]  # (the mangled name: ...<name>ENS_...)
        assert len(hits) == 1, (want, sorted(kernels))
        v = kernels[hits[0]]
        print(want, v)
        assert v.get("VGPRs Spill", 0) == 0 and v.get("SGPRs Spill", 0) == 0 and v["ScratchSize [bytes/lane]"] == 0, (want, v)
        assert v["VGPRs"] <= vgprs and v["LDS Size [bytes/block]"] <= 160 * 1024, (want, v)
    assert max(v["LDS Size [bytes/block]"] for v in kernels.values()) == 32 * 1024
