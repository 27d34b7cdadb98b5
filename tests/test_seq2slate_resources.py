"""hipcc's resource report for the Seq2Slate kernels (reagent_amd/csrc/seq2slate.hip): the expected kernels, no scratch and no
spilled registers, and the head's LDS image at S = 64 and E = 512 within the CU's 160 KB."""
from kernel_remarks import kernel_resources

PLAIN = ["s2s_embed_join_kernel", "s2s_embed_join_backward_kernel", "frechet_reduce_kernel"]
BY_WIDTH = ["frechet_head_kernel", "frechet_rank_kernel"]  # an instance per 1, 2, 4, 8 weight registers a lane (E <= 64 K)
EXP_TABLE = 15 * 8  # lstm_exp's constants


def test_kernels_have_no_scratch_and_no_spills(tmp_path):
    kernels = kernel_resources("seq2slate.hip", tmp_path)
    expected = [name + "E" for name in PLAIN] + [f"{name}ILi{k}E" for name in BY_WIDTH for k in (1, 2, 4, 8)]
    assert len(kernels) == len(expected), sorted(kernels)
    for want in expected:
        hits = [k for k in kernels if want in k]  # (the mangled name: ...<name>ENS_... / ...<name>ILi<K>EEE...)
        assert len(hits) == 1, (want, sorted(kernels))
        v = kernels[hits[0]]
        print(want, v)
        assert v.get("VGPRs Spill", 0) == 0 and v.get("SGPRs Spill", 0) == 0 and v["ScratchSize [bytes/lane]"] == 0, (want, v)
        assert v["VGPRs"] <= 256, (want, v)
        # the LDS images are static and sized for the limits (S = 64 candidates, E = 512 columns, four waves): the head's row of
        # d score per wave and the waves' sums of d w [512] and the four scalars, in double; the rank's keys and order per wave
        if want.startswith("frechet_head_kernel"):
            assert v["LDS Size [bytes/block]"] == 4 * 64 * 8 + 4 * (512 + 4) * 8 + EXP_TABLE <= 160 * 1024
        if want.startswith("frechet_rank_kernel"):
            assert v["LDS Size [bytes/block]"] == 4 * 64 * 8 + 4 * 64 * 4 + EXP_TABLE <= 160 * 1024
