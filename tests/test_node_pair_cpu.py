"""The child dwords of the f32 plane format (rtw_host.h pack_nodes32), on the host alone.

A node's 16-bit child codes {c0, c1} sit at dwords 24 and 26; dwords 25 and 27 hold the same two codes the other way round, {c1, c0}, so
that the 768-thread render builds read both orders with one 8-byte read at either per-ray offset and select the one whose low half is the
nearer child.  Checked here from the outside through rtw_bvh_dump and rtw_bvh_pack_nodes32: the straight dwords are the f16 nodes' codes
as they always were, the swapped ones are their halves exchanged, and every plane dword is the f16 plane, widened."""
import numpy as np
import pytest

import rtw_amd as R
from tests.test_bvh_builder_cpu import dump
from tests.test_node_format_cpu import hand_scene, layout, pack

TREES = {"2 spheres": (lambda: hand_scene(2), 1), "3 spheres": (lambda: hand_scene(3), 2), "book1": (lambda: R.Scene.generate(R.SCENE_C2), None)}      # (nodes, or None: Book-1 as the builder builds it, several hundred)


@pytest.fixture(scope="module", params=list(TREES))
def tree(request):
    make, n_nodes = TREES[request.param]
    d = dump(make())
    n16 = d["nodes16"]
    assert len(n16) == len(d["nodes"]) and n16.any(), "the scene must have f16 nodes"
    assert len(n16) == n_nodes if n_nodes else 400 < len(n16) <= 512
    return request.param, n16, pack(n16)


def codes(n16):
    """{c0, c1} of every node as the f32 plane format names them: a leaf keeps its code, an inner child index * 32 becomes index * code."""
    ch = n16[:, 12:14].astype(np.int16).astype(np.int64)
    want = np.where(ch >= 0, ch // 32 * layout()[3], ch) & 0xFFFF
    return ch, want


def test_the_trees_have_the_children_the_cases_need(tree):
    name, n16, _ = tree
    ch, _ = codes(n16)
    inner, leaf = ch >= 0, ch < 0
    if name == "2 spheres":
        assert leaf.all()                                        # one inner node over two leaves
    elif name == "3 spheres":
        assert (inner[:, 0] ^ inner[:, 1]).any()                 # a node with an inner child and a leaf child
    else:
        assert (inner[:, 0] & inner[:, 1]).any() and (leaf[:, 0] & leaf[:, 1]).any() and (inner[:, 0] ^ inner[:, 1]).any()


def test_straight_dwords_are_the_f16_codes(tree):
    _, n16, p = tree
    nd, ax, off, code = layout()
    _, want = codes(n16)
    word = (want[:, 0] | (want[:, 1] << 16)).astype(np.uint32)
    assert np.array_equal(p[:, 6 * ax], word) and np.array_equal(p[:, 6 * ax + off // 4], word)


def test_swapped_dwords_hold_the_same_halves_exchanged(tree):
    _, n16, p = tree
    nd, ax, off, code = layout()
    _, want = codes(n16)
    swapped = (want[:, 1] | (want[:, 0] << 16)).astype(np.uint32)
    for at in (6 * ax, 6 * ax + off // 4):                       # the pair a ray reads at its x offset: {straight, swapped}, 8-byte aligned
        assert at % 2 == 0 and at + 2 <= nd
        assert np.array_equal(p[:, at + 1], swapped)
        assert np.array_equal(p[:, at + 1] & 0xFFFF, p[:, at] >> 16) and np.array_equal(p[:, at + 1] >> 16, p[:, at] & 0xFFFF)


def test_every_plane_dword_is_the_f16_plane_widened(tree):
    _, n16, p = tree
    nd, ax, off, code = layout()
    planes = n16[:, :12].view(np.float16).astype(np.float32).reshape(-1, 2, 3, 2)      # [node][box][axis]{lo, hi}, exact widening
    want = np.empty((len(n16), 6 * ax), np.uint32)
    for c in range(2):
        for k in range(3):
            lo, hi = planes[:, c, k, 0].view(np.uint32), planes[:, c, k, 1].view(np.uint32)
            for j, w in enumerate([hi, lo, lo, hi]):
                want[:, (c * 3 + k) * ax + j] = w
    assert np.array_equal(p[:, :6 * ax], want)
    assert nd == 6 * ax + 4                                       # planes and the four child dwords: nothing else in a node
