"""Host side of the residual blocks (arch tokens RES / SKIP / SKIPL): the ResNet-CTC recipe generators against the
reference files held in tests/golden/reference_recipes.json, the recipe's parameter and LayerNorm counts and its output length, the
parameter order, numBlocks, every refusal, the streaming refusal and the recipe's flags file.  No GPU.

The four counts were worked out from the arch lines, not read off the build.  A `C cin cout 3 ...` line holds 3 cin cout + cout
parameters and a `C cin cout 1 ...` line cin cout + cout:
  am_resnet_ctc.arch           front 80 -> 1024; 8 blocks x 3 at 1024; 1024 -> 2048; 2 x 3 at 2048; 2048 -> 2304; 2 x 3 at 2304; one more
                               at 2304; output 2304 -> 9998 (k = 1): 306 268 430.  LayerNorms: one behind the front convolution, two
                               inside and one behind each of the 12 blocks, one behind each widening convolution and one in the
                               tail: 1 + 36 + 2 + 1 = 40
  am_resnet_ctc_librivox.arch  the same with 4096 for 2304 and a 4096 -> 512 bottleneck (k = 1) with a LayerNorm of its own in front of
                               512 -> 9998: 542 318 862 and 41 LayerNorms
  output length                T = 1500: the stride-2 SAME convolution gives 750, the three pools floor to 375, 187, 93."""
import json
import os

import pytest

from wav2letter_amd import _lib, recipes, streaming
from wav2letter_amd.trainer import Trainer, arch_check, flags_check

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "reference_recipes.json")
NFEAT, N = 8, 11
HEAD = "V -1 1 NFEAT 0\nC NFEAT 16 3 1 -1 1\n"
TAIL = "C 16 NLABEL 1 1 -1 1\nRO 2 0 3 1\n"


@pytest.fixture(scope="module")
def gold():
    with open(GOLD) as f:
        return json.load(f)


def cpu_trainer(arch, nfeat=NFEAT, nlabel=N):
    return Trainer(arch, nfeat, nlabel, "ctc", device="cpu")


@pytest.mark.parametrize("gen,kind,key", [(recipes.resnet_ctc_arch, "arch", "sota/2019/am_arch/am_resnet_ctc.arch"),
                                          (recipes.resnet_ctc_librivox_arch, "arch", "sota/2019/am_arch/am_resnet_ctc_librivox.arch"),
                                          (recipes.resnet_ctc_train_cfg, "cfg", "sota/2019/librispeech/train_am_resnet_ctc.cfg")])
def test_generators_reproduce_the_reference_files(gold, gen, kind, key):
    assert gen().splitlines() == gold[kind][key].splitlines()


def _counts(tr):
    table = tr.param_table()
    return sum(n for name, n, _ in table if not name.startswith("ln.")), sum(1 for name, _, _ in table if name.startswith("ln."))


def test_resnet_ctc_recipe_counts_and_output_length():
    arch = recipes.resnet_ctc_arch()
    assert arch_check(arch, 80, 9998) == len([l for l in arch.splitlines() if l and not l.startswith("#")])
    tr = cpu_trainer(arch, 80, 9998)
    assert _counts(tr) == (306268430, 40)
    assert tr.plan(2, 1500, 40) == 93
    assert tr.describe().count("Residual") == 12


def test_resnet_ctc_librivox_recipe_counts():
    assert _counts(cpu_trainer(recipes.resnet_ctc_librivox_arch(), 80, 9998)) == (542318862, 41)


def test_parameter_table_is_in_arch_line_order_with_the_projection_at_its_line():
    """the block's layers in arch-line order; the SKIPL projection where its line stands -- here between the block's two convolutions"""
    arch = HEAD + "RES 3 1 1\nC 16 24 3 1 -1 1\nSKIPL 0 4 2 0.5\nC 16 20 1 1 -1 1\nL 20 24\nR\nC 24 24 5 1 -1 1\n" + TAIL.replace("C 16", "C 24")
    with pytest.raises(_lib.W2LInvalidArgument):     # (an L on a convolution layout: the projection's own layers are checked like any other)
        cpu_trainer(arch)
    arch = HEAD + "RES 3 1 1\nC 16 24 3 1 -1 1\nSKIPL 0 4 2 0.5\nC 16 20 1 1 -1 1\nC 20 24 1 1 -1 1\nR\nC 24 24 5 1 -1 1\n" + TAIL.replace("C 16", "C 24")
    got = [(name, n) for name, n, _ in cpu_trainer(arch).param_table()]
    want = [("conv.w", 3 * 8 * 16), ("conv.b", 16),                       # HEAD
            ("conv.w", 3 * 16 * 24), ("conv.b", 24),                      # the block's first convolution
            ("conv.w", 16 * 20), ("conv.b", 20), ("conv.w", 20 * 24), ("conv.b", 24),   # the projection, at its SKIPL line
            ("conv.w", 5 * 24 * 24), ("conv.b", 24),                      # the block's second convolution
            ("conv.w", 24 * 11), ("conv.b", 11)]
    assert got == want
    # ... and at the end of the block when its line stands there
    arch = HEAD + "RES 3 1 1\nC 16 24 3 1 -1 1\nR\nC 24 24 5 1 -1 1\nSKIPL 0 4 1\nC 16 24 1 1 -1 1\n" + TAIL.replace("C 16", "C 24")
    got = [n for _, n, _ in cpu_trainer(arch).param_table()]
    assert got == [384, 16, 1152, 24, 2880, 24, 384, 24, 264, 11]


def test_numblocks_builds_blocks_with_parameters_of_their_own():
    arch = HEAD + "RES 2 1 2\nC 16 16 3 1 -1 1\nR\nSKIP 0 3 0.5\n" + TAIL
    tr = cpu_trainer(arch)
    assert tr.describe().count("Residual") == 2
    table = tr.param_table()
    assert [n for _, n, _ in table] == [384, 16, 768, 16, 768, 16, 176, 11]
    offs = [off for _, _, off in table]
    assert len(set(offs)) == len(offs) and offs == sorted(offs)
    # the lines are counted once: what follows the block is the next layer, and the count without numBlocks is one block
    assert cpu_trainer(HEAD + "RES 2 1 1\nC 16 16 3 1 -1 1\nR\nSKIP 0 3 0.5\n" + TAIL).describe().count("Residual") == 1
    # a PD line counts as a line and folds into its convolution inside the block as outside
    pd = cpu_trainer(HEAD + "RES 2 1 1\nPD 0 1 1\nC 16 16 3 1 0 1\nSKIP 0 3\n" + TAIL)
    assert [n for _, n, _ in pd.param_table()] == [384, 16, 768, 16, 176, 11] and pd.plan(1, 50, 5) == 50


REFUSED = [
    ("RES 2 1 1\nC 16 16 3 1 -1 1\nR\nSKIP 1 3\n" + TAIL, r"from = 0.*SKIP 1 3.*RES 2 1 1"),
    ("RES 2 1 1\nC 16 16 3 1 -1 1\nR\nSKIP 0 2\n" + TAIL, r"to = numLayers \+ 1 = 3.*SKIP 0 2.*RES 2 1 1"),
    ("RES 2 1 1\nC 16 16 3 1 -1 1\nR\nSKIPL 0 4 1\nC 16 16 1 1 -1 1\n" + TAIL, r"to = numLayers \+ 1 = 3.*SKIPL 0 4 1"),
    ("RES 2 2 1\nC 16 16 3 1 -1 1\nR\nSKIP 0 3\nSKIP 0 3\n" + TAIL, r"more than one shortcut.*SKIP 0 3.*RES 2 2 1"),
    ("RES 2 0 1\nC 16 16 3 1 -1 1\nR\n" + TAIL, r"without a shortcut.*RES 2 0 1"),
    ("RES 2 1 1\nC 16 16 3 1 -1 1\n", r"the file ends inside 'RES 2 1 1'"),
    ("RES 2 1 1\nC 16 16 3 1 -1 1\nR\nSKIPL 0 3 2\nC 16 16 1 1 -1 1\n", r"the file ends inside the projection of 'RES 2 1 1'"),
    ("RES 2 1 0\nC 16 16 3 1 -1 1\nR\nSKIP 0 3\n" + TAIL, r"Invalid number of residual blocks: 0.*RES 2 1 0"),
    ("RES 2 1 -2\nC 16 16 3 1 -1 1\nR\nSKIP 0 3\n" + TAIL, r"Invalid number of residual blocks: -2"),
    ("RES 2 1\nC 16 16 3 1 -1 1\nR\nSKIP 0 3\n" + TAIL, r"Failed parsing - RES 2 1"),
    ("RES 2 1 1\nC 16 16 3 1 -1 1\nR\nSKIP 0\n" + TAIL, r"Failed parsing - SKIP 0"),
    ("RES 2 1 1\nC 16 16 3 1 -1 1\nR\nSKIP 0 3 0.5 7\n" + TAIL, r"Failed parsing - SKIP 0 3 0.5 7"),
    ("RES 2 1 1\nC 16 16 3 1 -1 1\nR\nSKIPL 0 3\n" + TAIL, r"Failed parsing - SKIPL 0 3"),
    ("RES 2 1 1\nC 16 24 3 1 -1 1\nR\nSKIP 0 3\n" + TAIL.replace("C 16", "C 24"), r"differ in shape or layout.*SKIP 0 3.*RES 2 1 1"),
    ("RES 2 1 1\nC 16 16 3 1 -1 1\nRO 2 0 3 1\nSKIP 0 3\nRO 1 3 0 2\n" + TAIL, r"differ in shape or layout"),
    ("RES 4 1 1\nRES 2 1 1\nC 16 16 3 1 -1 1\nR\nSKIP 0 3\nSKIP 0 5\n" + TAIL, r"inside a residual block"),
    ("SKIP 0 3\n" + TAIL, r"outside the lines a RES block announces"),
    ("RES 2 1 1\nC 16 16 3 1 -1 1\nPD 0 1 1\nSKIP 0 3\n" + TAIL, r"dangling PD"),
    ("RES 2 1 1\nWN 3 AC 16 16 5 1 -1 0\nR\nSKIP 0 3\n" + TAIL, r"layer 'AC' is outside the hot path"),
]


@pytest.mark.parametrize("body,message", REFUSED, ids=[str(i) for i in range(len(REFUSED))])
def test_refusals_name_the_line(body, message):
    with pytest.raises(_lib.W2LInvalidArgument, match=message):
        cpu_trainer(HEAD + body)


def test_convlm_archs_still_fail_at_their_ac_line(gold):
    """every child that was refused stays refused: the ConvLM / gated-CNN language models now get as far as their first AC line"""
    keys = [k for k in gold["arch"] if "convlm" in k or "gcnn" in k]
    assert len(keys) >= 7
    for k in keys:
        with pytest.raises(_lib.W2LInvalidArgument, match=r"layer '(AC|E|ADAPTIVEE)' is outside the hot path"):
            cpu_trainer(gold["arch"][k], 1, 100)


def test_streaming_session_refuses_and_names_the_res_line():
    arch = HEAD + "RES 2 1 1\nC 16 16 3 1 -1 1\nR\nSKIP 0 3 0.5\n" + TAIL
    with pytest.raises(_lib.W2LError, match=r"arch line 'RES 2 1 1' \(Residual\) cannot be streamed"):
        streaming.query(arch, NFEAT, N, 2, 8)


def test_resnet_cfg_parses(gold):
    """the reference's train_am_resnet_ctc.cfg parses as it stands (30 flags; --labelsmooth, --sampletarget, --mintsz and --minisz
    are carried and not read: INTEGRATION.md)"""
    assert flags_check(recipes.resnet_ctc_train_cfg()) == 30
    assert flags_check(gold["cfg"]["sota/2019/librispeech/train_am_resnet_ctc.cfg"]) == 30
