"""Cases of the exact tests of the first stage without its convolution output (csrc/first_stage.hip;
tests/first_stage_exact.py, test_first_stage_exact_host.py, test_gpu_first_stage_exact.py).  Data only.

Every x is (N, 8, H, W), every convolution 3x3 'same'.  A case lists what it is there for as numbers the host test
recomputes from the restated plan of tests/first_stage_exact.py and holds to the library's byte queries:
  blocks   N * (H / 8) * (W / 64), the 8-row x 64-column blocks the persistent workgroups walk
  gram     (fewest, most) blocks one fs_gram_kernel workgroup walks; ragged when they differ
  wgrad    the same for fs_wgrad_kernel
  chunks   lengths of the reduction chunks of fs_reduce_kernel (elements of one channel)
  form     the fs_wgrad_kernel<NTW, DQ> instantiation, fixed by (algebra, Cout)
  bias     False: the convolution has none (bias = NULL);  drop: run with drop_p = 0.5 as well
  sections which of A (gram), B (bn), C (backward) run the case"""


def _c(name, x, cout, algebra, blocks, gram, wgrad, chunks, form, sections="ABC", bias=True, drop=False, why=""):
    return dict(name=name, x=tuple(x), cout=cout, algebra=algebra, blocks=blocks, gram=tuple(gram), wgrad=tuple(wgrad),
                chunks=tuple(chunks), form=form, sections=sections, bias=bias, drop=drop, why=why,
                k=(3, 3), stride=1, padding=1, dilation=1)


CASES = [
    _c("one_block_q64", (1, 8, 8, 64), 64, 4, 1, (1, 1), (1, 1), (64,), "<2, false>", drop=True,
       why="one block: all four borders of the tile lie outside the image; quaternion block table"),
    _c("one_block_dq64", (1, 8, 8, 64), 64, 8, 1, (1, 1), (1, 1), (64,), "<2, true>", bias=False,
       why="one block, dual quaternion at 64 channels: <2, true>; no convolution bias"),
    _c("one_block_r64", (1, 8, 8, 64), 64, 1, 1, (1, 1), (1, 1), (64,), "<2, false>",
       why="one block, algebra 1: the weight itself is the real matrix"),
    _c("halos_dq128", (2, 8, 16, 128), 128, 8, 8, (1, 1), (1, 1), (512,), "<4, true>", drop=True,
       why="interior halos in both directions, an image boundary between blocks; <4, true>"),
    _c("halos_dq192", (2, 8, 16, 128), 192, 8, 8, (1, 1), (1, 1), (512,), "<6, true>",
       why="the same blocks at 192 channels: <6, true>"),
    _c("ragged_wgrad_q64", (5, 8, 8, 5120), 64, 4, 400, (1, 1), (1, 2), (8536, 8536, 8528), "<2, false>",
       why="400 blocks: 144 wgrad workgroups walk 2 blocks, 112 walk 1; three reduction chunks, the last short"),
    _c("ragged_wgrad_dq64", (5, 8, 8, 5120), 64, 8, 400, (1, 1), (1, 2), (8536, 8536, 8528), "<2, true>",
       why="the same with the dual quaternion's narrow tiles"),
    _c("ragged_gram_q64", (3, 8, 24, 3712), 64, 4, 522, (1, 2), (2, 3), (8352, 8352, 8352, 8352), "<2, false>",
       why="522 blocks: 10 Gram workgroups walk 2 blocks; wgrad 3 / 2 blocks, the LDS buffer toggle returns to 0"),
    _c("ragged_gram_dq192", (3, 8, 24, 3712), 192, 8, 522, (1, 2), (2, 3), (8352, 8352, 8352, 8352), "<6, true>",
       why="the same at 192 channels"),
    _c("three_gram_blocks", (1, 8, 8, 64 * 1030), 64, 4, 1030, (2, 3), (4, 5), (8240,) * 8, "<2, false>", sections="A",
       why="1030 blocks: 6 Gram workgroups walk three blocks (two cross-block prefetches)"),
]
BY_NAME = {c["name"]: c for c in CASES}
assert len(BY_NAME) == len(CASES)
