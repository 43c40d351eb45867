"""What dmb_deconv3d_k3s2_f32 runs for a launch (csrc/deconv3d_plan.h: deconv_plan), seen through the query
dmb_deconv3d_k3s2_plan: a pure host function, so this runs without a GPU.  The estimate counts workgroup slots over the device's
compute units: 256, the MI355X's, which is also what the library assumes without a device.

The expected codes were RECORDED FROM THE LIBRARY BEFORE THE PLAN EXISTED: a print of the chosen instantiation in each of its three
launch functions (and the refusals' codes and messages), for launches made with made-up pointers of the given alignments.  A change
that moves a choice, a threshold or a refusal shows here.

Plan code = (form << 8) | tile: form 1 = split-K, 2 = work queue (tile 0 = 28, 1 = 32, 2 = 64 columns; + 4 for 64 output channels),
3 = two-parity (0 = 60 columns dword, 1 = 60 columns 16-byte staging, 2 = + 16-byte epilogue, 3 / 4 = 2 x 28 columns with the
8- / 16-byte epilogue; + 5 for 64 output channels); a refusal is minus its DMB_E* code."""
import types

import pytest

from densematchingbenchmark_amd import _lib, ops

EINVAL, EUNSUPPORTED = 100001, 100002
NCU = 256

# (what the row is there for, B, Ci, Co, D, H, W, Wout, alignment of x / y / residual / workspace (0 = none), single-chain flag,
#  recorded plan code, recorded message of a refusal)
CASES = [
    ("split-K", 1, 32, 32, 2, 4, 16, 32, 16, 16, 16, 16, 0, 0x100, ""),
    ("split-K Co 64", 1, 16, 64, 1, 1, 4, 8, 16, 16, 16, 16, 0, 0x100, ""),
    ("split-K Co 1", 1, 8, 1, 1, 1, 4, 8, 16, 16, 16, 16, 0, 0x100, ""),
    ("queue 32 N28", 1, 32, 32, 2, 3, 80, 160, 16, 16, 16, 16, 1, 0x200, ""),
    ("queue 32 F32", 1, 32, 32, 2, 3, 32, 64, 16, 16, 16, 16, 1, 0x201, ""),
    ("queue 32 F64", 1, 32, 32, 2, 3, 64, 128, 16, 16, 16, 16, 1, 0x202, ""),
    ("queue 64 N28 (padded rows)", 1, 32, 64, 2, 3, 80, 156, 16, 16, 16, 16, 1, 0x204, ""),
    ("queue 64 F32 (padded rows)", 1, 32, 64, 2, 3, 32, 60, 16, 16, 16, 16, 1, 0x205, ""),
    ("queue 64 F64 (padded rows)", 1, 32, 64, 2, 3, 64, 124, 16, 16, 16, 16, 1, 0x206, ""),
    ("parity 32 dword", 1, 8, 32, 2, 3, 13, 26, 16, 16, 16, 16, 0, 0x300, ""),
    ("parity 32 W60 v16", 1, 32, 32, 2, 3, 32, 64, 16, 8, 16, 16, 1, 0x301, ""),
    ("parity 32 W60 vepi", 1, 32, 32, 2, 3, 32, 64, 16, 16, 16, 0, 1, 0x302, ""),
    ("parity 32 N28 v16", 1, 32, 32, 2, 3, 64, 128, 16, 8, 16, 16, 1, 0x303, ""),
    ("parity 32 N28 vepi", 1, 32, 32, 2, 3, 64, 128, 16, 16, 16, 0, 1, 0x304, ""),
    ("parity 64 dword", 1, 8, 64, 2, 3, 13, 26, 16, 16, 16, 16, 0, 0x305, ""),
    ("parity 64 W60 v16", 1, 32, 64, 2, 3, 32, 64, 16, 16, 4, 16, 1, 0x306, ""),
    ("parity 64 W60 vepi", 1, 32, 64, 2, 3, 32, 64, 16, 16, 16, 16, 1, 0x307, ""),
    ("parity 64 N28 v16", 1, 32, 64, 2, 3, 64, 128, 16, 4, 16, 16, 1, 0x308, ""),
    ("parity 64 N28 vepi", 1, 32, 64, 2, 3, 64, 128, 16, 16, 16, 16, 1, 0x309, ""),
    ("split-K 1280 units", 1, 32, 32, 1, 2560, 16, 32, 16, 16, 16, 16, 0, 0x100, ""),
    ("split-K 1281 units", 1, 32, 32, 1, 2562, 16, 32, 16, 16, 16, 16, 0, 0x200, ""),
    ("split-K 1280 units Co 64", 1, 64, 64, 1, 1280, 16, 32, 16, 16, 16, 16, 0, 0x100, ""),
    ("split-K 1282 units Co 64", 1, 64, 64, 1, 1282, 16, 32, 16, 16, 16, 16, 0, 0x204, ""),
    ("split-K 1280 units no ws", 1, 32, 32, 1, 2560, 16, 32, 16, 16, 16, 0, 0, 0x100, ""),
    ("split-K 1281 units no ws", 1, 32, 32, 1, 2562, 16, 32, 16, 16, 16, 0, 0, 0x304, ""),
    ("split-K W % 4", 1, 32, 32, 2, 4, 18, 36, 16, 16, 16, 16, 0, 0x300, ""),
    ("split-K x align 8", 1, 32, 32, 2, 4, 16, 32, 8, 16, 16, 16, 0, 0x300, ""),
    ("split-K y align 4", 1, 32, 32, 2, 4, 16, 32, 16, 4, 16, 16, 0, 0x303, ""),
    ("split-K res align 8", 1, 32, 32, 2, 4, 16, 32, 16, 16, 8, 16, 0, 0x303, ""),
    ("split-K padded rows", 1, 32, 32, 2, 4, 16, 28, 16, 16, 16, 16, 0, 0x100, ""),
    ("split-K padded rows no ws", 1, 32, 32, 2, 4, 16, 28, 16, 16, 16, 0, 0, 0x100, ""),
    ("single chain small", 1, 32, 32, 2, 4, 16, 32, 16, 16, 16, 16, 1, 0x200, ""),
    ("single chain small no ws", 1, 32, 32, 2, 4, 16, 32, 16, 16, 16, 0, 1, 0x304, ""),
    ("slot rule 960 items", 1, 64, 64, 8, 60, 32, 64, 16, 16, 16, 16, 1, 0x307, ""),
    ("slot rule 976 items", 1, 64, 64, 8, 61, 32, 64, 16, 16, 16, 16, 1, 0x205, ""),
    ("slot rule 960 items narrow", 1, 64, 64, 8, 20, 80, 160, 16, 16, 16, 16, 1, 0x309, ""),
    ("slot rule 1008 items narrow", 1, 64, 64, 8, 21, 80, 160, 16, 16, 16, 16, 1, 0x204, ""),
    ("slot rule Co 32 exempt", 1, 64, 32, 8, 60, 32, 64, 16, 16, 16, 16, 1, 0x201, ""),
    ("slot rule padded exempt", 1, 64, 64, 8, 60, 32, 60, 16, 16, 16, 16, 1, 0x205, ""),
    ("slot rule 960 items, split-K first", 1, 64, 64, 8, 60, 32, 64, 16, 16, 16, 16, 0, 0x100, ""),
    ("slot rule: conv5 of one 544x960 pair", 1, 64, 64, 12, 34, 60, 120, 16, 16, 16, 16, 0, 0x307, ""),
    ("conv5 of two pairs", 2, 64, 64, 12, 34, 60, 120, 16, 16, 16, 16, 0, 0x206, ""),
    ("width 32 Co 32", 2, 64, 32, 8, 64, 32, 64, 16, 16, 16, 16, 1, 0x201, ""),
    ("width 32 Co 64", 2, 64, 64, 8, 64, 32, 64, 16, 16, 16, 16, 1, 0x205, ""),
    ("width 32 Co 32 no ws", 2, 64, 32, 8, 64, 32, 64, 16, 16, 16, 0, 1, 0x302, ""),
    ("width 32 Co 64 no ws", 2, 64, 64, 8, 64, 32, 64, 16, 16, 16, 0, 1, 0x307, ""),
    ("width 40 Co 32", 2, 64, 32, 8, 64, 40, 80, 16, 16, 16, 16, 1, 0x202, ""),
    ("width 40 Co 64", 2, 64, 64, 8, 64, 40, 80, 16, 16, 16, 16, 1, 0x206, ""),
    ("width 40 Co 32 no ws", 2, 64, 32, 8, 64, 40, 80, 16, 16, 16, 0, 1, 0x302, ""),
    ("width 40 Co 64 no ws", 2, 64, 64, 8, 64, 40, 80, 16, 16, 16, 0, 1, 0x307, ""),
    ("width 64 Co 32", 2, 64, 32, 8, 64, 64, 128, 16, 16, 16, 16, 1, 0x202, ""),
    ("width 64 Co 64", 2, 64, 64, 8, 64, 64, 128, 16, 16, 16, 16, 1, 0x206, ""),
    ("width 64 Co 32 no ws", 2, 64, 32, 8, 64, 64, 128, 16, 16, 16, 0, 1, 0x304, ""),
    ("width 64 Co 64 no ws", 2, 64, 64, 8, 64, 64, 128, 16, 16, 16, 0, 1, 0x309, ""),
    ("width 80 Co 32", 2, 64, 32, 8, 64, 80, 160, 16, 16, 16, 16, 1, 0x200, ""),
    ("width 80 Co 64", 2, 64, 64, 8, 64, 80, 160, 16, 16, 16, 16, 1, 0x204, ""),
    ("width 80 Co 32 no ws", 2, 64, 32, 8, 64, 80, 160, 16, 16, 16, 0, 1, 0x304, ""),
    ("width 80 Co 64 no ws", 2, 64, 64, 8, 64, 80, 160, 16, 16, 16, 0, 1, 0x309, ""),
    ("width 84 Co 32", 2, 64, 32, 8, 64, 84, 168, 16, 16, 16, 16, 1, 0x200, ""),
    ("width 84 Co 64", 2, 64, 64, 8, 64, 84, 168, 16, 16, 16, 16, 1, 0x204, ""),
    ("width 84 Co 32 no ws", 2, 64, 32, 8, 64, 84, 168, 16, 16, 16, 0, 1, 0x304, ""),
    ("width 84 Co 64 no ws", 2, 64, 64, 8, 64, 84, 168, 16, 16, 16, 0, 1, 0x309, ""),
    ("width 88 Co 32", 2, 64, 32, 8, 64, 88, 176, 16, 16, 16, 16, 1, 0x201, ""),
    ("width 88 Co 64", 2, 64, 64, 8, 64, 88, 176, 16, 16, 16, 16, 1, 0x205, ""),
    ("width 88 Co 32 no ws", 2, 64, 32, 8, 64, 88, 176, 16, 16, 16, 0, 1, 0x302, ""),
    ("width 88 Co 64 no ws", 2, 64, 64, 8, 64, 88, 176, 16, 16, 16, 0, 1, 0x307, ""),
    ("width 120 Co 32", 2, 64, 32, 8, 64, 120, 240, 16, 16, 16, 16, 1, 0x202, ""),
    ("width 120 Co 64", 2, 64, 64, 8, 64, 120, 240, 16, 16, 16, 16, 1, 0x206, ""),
    ("width 120 Co 32 no ws", 2, 64, 32, 8, 64, 120, 240, 16, 16, 16, 0, 1, 0x302, ""),
    ("width 120 Co 64 no ws", 2, 64, 64, 8, 64, 120, 240, 16, 16, 16, 0, 1, 0x307, ""),
    ("width 156 Co 32", 2, 64, 32, 8, 64, 156, 312, 16, 16, 16, 16, 1, 0x201, ""),
    ("width 156 Co 64", 2, 64, 64, 8, 64, 156, 312, 16, 16, 16, 16, 1, 0x205, ""),
    ("width 156 Co 32 no ws", 2, 64, 32, 8, 64, 156, 312, 16, 16, 16, 0, 1, 0x302, ""),
    ("width 156 Co 64 no ws", 2, 64, 64, 8, 64, 156, 312, 16, 16, 16, 0, 1, 0x307, ""),
    ("width 60 Co 32", 2, 64, 32, 8, 64, 60, 120, 16, 16, 16, 16, 1, 0x202, ""),
    ("width 60 Co 64", 2, 64, 64, 8, 64, 60, 120, 16, 16, 16, 16, 1, 0x206, ""),
    ("width 60 Co 32 no ws", 2, 64, 32, 8, 64, 60, 120, 16, 16, 16, 0, 1, 0x302, ""),
    ("width 60 Co 64 no ws", 2, 64, 64, 8, 64, 60, 120, 16, 16, 16, 0, 1, 0x307, ""),
    ("width 28 Co 32", 2, 64, 32, 8, 64, 28, 56, 16, 16, 16, 16, 1, 0x200, ""),
    ("width 28 Co 64", 2, 64, 64, 8, 64, 28, 56, 16, 16, 16, 16, 1, 0x204, ""),
    ("width 28 Co 32 no ws", 2, 64, 32, 8, 64, 28, 56, 16, 16, 16, 0, 1, 0x304, ""),
    ("width 28 Co 64 no ws", 2, 64, 64, 8, 64, 28, 56, 16, 16, 16, 0, 1, 0x309, ""),
    ("width 4 Co 32", 2, 64, 32, 8, 64, 4, 8, 16, 16, 16, 16, 1, 0x200, ""),
    ("width 4 Co 64", 2, 64, 64, 8, 64, 4, 8, 16, 16, 16, 16, 1, 0x204, ""),
    ("width 4 Co 32 no ws", 2, 64, 32, 8, 64, 4, 8, 16, 16, 16, 0, 1, 0x304, ""),
    ("width 4 Co 64 no ws", 2, 64, 64, 8, 64, 4, 8, 16, 16, 16, 0, 1, 0x309, ""),
    ("Ci 16 small", 1, 16, 32, 2, 4, 32, 64, 16, 16, 16, 16, 0, 0x100, ""),
    ("Ci 16 large", 2, 16, 32, 8, 64, 64, 128, 16, 16, 16, 16, 0, 0x304, ""),
    ("Ci 16 large Co 64", 2, 16, 64, 8, 64, 64, 128, 16, 16, 16, 16, 0, 0x309, ""),
    ("Ci 16 single chain", 1, 16, 32, 2, 4, 32, 64, 16, 16, 16, 16, 1, 0x302, ""),
    ("Ci 24 small", 1, 24, 32, 2, 4, 32, 64, 16, 16, 16, 16, 0, 0x100, ""),
    ("Ci 24 large", 2, 24, 32, 8, 64, 64, 128, 16, 16, 16, 16, 0, 0x304, ""),
    ("Ci 24 large Co 64", 2, 24, 64, 8, 64, 64, 128, 16, 16, 16, 16, 0, 0x309, ""),
    ("Ci 24 single chain", 1, 24, 32, 2, 4, 32, 64, 16, 16, 16, 16, 1, 0x302, ""),
    ("Ci 32 small", 1, 32, 32, 2, 4, 32, 64, 16, 16, 16, 16, 0, 0x100, ""),
    ("Ci 32 large", 2, 32, 32, 8, 64, 64, 128, 16, 16, 16, 16, 0, 0x202, ""),
    ("Ci 32 large Co 64", 2, 32, 64, 8, 64, 64, 128, 16, 16, 16, 16, 0, 0x206, ""),
    ("Ci 32 single chain", 1, 32, 32, 2, 4, 32, 64, 16, 16, 16, 16, 1, 0x201, ""),
    ("Ci 48 small", 1, 48, 32, 2, 4, 32, 64, 16, 16, 16, 16, 0, 0x100, ""),
    ("Ci 48 large", 2, 48, 32, 8, 64, 64, 128, 16, 16, 16, 16, 0, 0x202, ""),
    ("Ci 48 large Co 64", 2, 48, 64, 8, 64, 64, 128, 16, 16, 16, 16, 0, 0x206, ""),
    ("Ci 48 single chain", 1, 48, 32, 2, 4, 32, 64, 16, 16, 16, 16, 1, 0x201, ""),
    ("Ci 72 small", 1, 72, 32, 2, 4, 32, 64, 16, 16, 16, 16, 0, 0x302, ""),
    ("Ci 72 large", 2, 72, 32, 8, 64, 64, 128, 16, 16, 16, 16, 0, 0x304, ""),
    ("Ci 72 large Co 64", 2, 72, 64, 8, 64, 64, 128, 16, 16, 16, 16, 0, 0x309, ""),
    ("Ci 72 single chain", 1, 72, 32, 2, 4, 32, 64, 16, 16, 16, 16, 1, 0x302, ""),
    ("Co 1 small", 1, 32, 1, 2, 4, 32, 64, 16, 16, 16, 16, 0, 0x100, ""),
    ("Co 1 large", 2, 32, 1, 8, 64, 64, 128, 16, 16, 16, 16, 0, 0x303, ""),
    ("Co 1 large no ws", 2, 32, 1, 8, 64, 64, 128, 16, 16, 16, 0, 0, 0x303, ""),
    ("Co 1 odd width", 2, 32, 1, 8, 64, 35, 70, 16, 16, 16, 16, 0, 0x300, ""),
    ("Co 32 small", 1, 32, 32, 2, 4, 32, 64, 16, 16, 16, 16, 0, 0x100, ""),
    ("Co 32 large", 2, 32, 32, 8, 64, 64, 128, 16, 16, 16, 16, 0, 0x202, ""),
    ("Co 32 large no ws", 2, 32, 32, 8, 64, 64, 128, 16, 16, 16, 0, 0, 0x304, ""),
    ("Co 32 odd width", 2, 32, 32, 8, 64, 35, 70, 16, 16, 16, 16, 0, 0x300, ""),
    ("Co 64 small", 1, 32, 64, 2, 4, 32, 64, 16, 16, 16, 16, 0, 0x100, ""),
    ("Co 64 large", 2, 32, 64, 8, 64, 64, 128, 16, 16, 16, 16, 0, 0x206, ""),
    ("Co 64 large no ws", 2, 32, 64, 8, 64, 64, 128, 16, 16, 16, 0, 0, 0x309, ""),
    ("Co 64 odd width", 2, 32, 64, 8, 64, 35, 70, 16, 16, 16, 16, 0, 0x305, ""),
    ("x align 4", 2, 32, 32, 8, 64, 64, 128, 4, 16, 16, 16, 0, 0x300, ""),
    ("y align 4", 2, 32, 32, 8, 64, 64, 128, 16, 4, 16, 16, 0, 0x303, ""),
    ("res align 4", 2, 32, 64, 8, 64, 120, 240, 16, 16, 4, 16, 0, 0x306, ""),
    ("x align 4 no ws", 2, 32, 64, 8, 64, 120, 240, 4, 16, 16, 0, 0, 0x305, ""),
    ("ws align 4", 2, 32, 32, 8, 64, 64, 128, 16, 16, 16, 4, 0, 0x202, ""),
    ("x align 8", 2, 32, 32, 8, 64, 64, 128, 8, 16, 16, 16, 0, 0x300, ""),
    ("y align 8", 2, 32, 32, 8, 64, 64, 128, 16, 8, 16, 16, 0, 0x303, ""),
    ("res align 8", 2, 32, 64, 8, 64, 120, 240, 16, 16, 8, 16, 0, 0x306, ""),
    ("x align 8 no ws", 2, 32, 64, 8, 64, 120, 240, 8, 16, 16, 0, 0, 0x305, ""),
    ("ws align 8", 2, 32, 32, 8, 64, 64, 128, 16, 16, 16, 8, 0, 0x202, ""),
    ("x align 16", 2, 32, 32, 8, 64, 64, 128, 16, 16, 16, 16, 0, 0x202, ""),
    ("y align 16", 2, 32, 32, 8, 64, 64, 128, 16, 16, 16, 16, 0, 0x202, ""),
    ("res align 16", 2, 32, 64, 8, 64, 120, 240, 16, 16, 16, 16, 0, 0x206, ""),
    ("x align 16 no ws", 2, 32, 64, 8, 64, 120, 240, 16, 16, 16, 0, 0, 0x307, ""),
    ("ws align 16", 2, 32, 32, 8, 64, 64, 128, 16, 16, 16, 16, 0, 0x202, ""),
    ("misaligned workspace", 2, 32, 32, 8, 64, 64, 128, 16, 16, 16, 2, 0, -EINVAL, "deconv3d: misaligned workspace"),
    ("misaligned workspace, shape not for the queue", 2, 8, 32, 8, 64, 13, 26, 16, 16, 16, 2, 0, -EINVAL, "deconv3d: misaligned workspace"),
    ("misaligned workspace, split-K first", 1, 32, 32, 2, 4, 16, 32, 16, 16, 16, 2, 0, 0x100, ""),
    ("misaligned workspace, byte", 2, 32, 32, 8, 64, 64, 128, 16, 16, 16, 1, 0, -EINVAL, "deconv3d: misaligned workspace"),
    ("padded rows", 2, 64, 64, 3, 5, 80, 156, 16, 16, 16, 16, 1, 0x204, ""),
    ("padded rows no ws", 2, 64, 64, 3, 5, 80, 156, 16, 16, 16, 0, 1, -EUNSUPPORTED, "deconv3d: a row-padded input (Wout < 2 W) needs the workspace form: Co 32 or 64, Ci % 16 == 0, Wout % 4 == 0, aligned operands"),
    ("padded rows Co 32", 1, 64, 32, 4, 6, 132, 260, 16, 16, 16, 16, 1, 0x200, ""),
    ("padded rows Ci 16", 1, 16, 32, 4, 6, 132, 260, 16, 16, 16, 16, 1, -EUNSUPPORTED, "deconv3d: a row-padded input (Wout < 2 W) needs the workspace form: Co 32 or 64, Ci % 16 == 0, Wout % 4 == 0, aligned operands"),
    ("padded rows Ci 48", 1, 48, 32, 4, 6, 132, 260, 16, 16, 16, 16, 1, 0x200, ""),
    ("padded rows Co 1", 1, 32, 1, 4, 6, 132, 260, 16, 16, 16, 16, 1, -EUNSUPPORTED, "deconv3d: a row-padded input (Wout < 2 W) needs the workspace form: Co 32 or 64, Ci % 16 == 0, Wout % 4 == 0, aligned operands"),
    ("padded rows x align 8", 1, 32, 32, 4, 6, 132, 260, 8, 16, 16, 16, 1, -EUNSUPPORTED, "deconv3d: a row-padded input (Wout < 2 W) needs the workspace form: Co 32 or 64, Ci % 16 == 0, Wout % 4 == 0, aligned operands"),
    ("padded rows Wout 2 W - 2", 1, 32, 32, 4, 6, 132, 262, 16, 16, 16, 16, 1, -EUNSUPPORTED, "deconv3d: a row-padded input (Wout < 2 W) needs the workspace form: Co 32 or 64, Ci % 16 == 0, Wout % 4 == 0, aligned operands"),
    ("padded rows Wout 2 W - 6", 1, 32, 32, 4, 6, 132, 258, 16, 16, 16, 16, 1, -EUNSUPPORTED, "deconv3d: a row-padded input (Wout < 2 W) needs the workspace form: Co 32 or 64, Ci % 16 == 0, Wout % 4 == 0, aligned operands"),
    ("padded rows large", 4, 64, 64, 12, 34, 80, 156, 16, 16, 16, 16, 0, 0x204, ""),
    ("B = 0", 0, 32, 32, 2, 4, 16, 32, 16, 16, 16, 16, 0, -EINVAL, "deconv3d: bad argument"),
    ("Ci = 0", 1, 0, 32, 2, 4, 16, 32, 16, 16, 16, 16, 0, -EINVAL, "deconv3d: bad argument"),
    ("W = 0", 1, 32, 32, 2, 4, 0, 0, 16, 16, 16, 16, 0, -EINVAL, "deconv3d: bad argument"),
    ("Wout odd", 1, 32, 32, 2, 4, 16, 31, 16, 16, 16, 16, 0, -EINVAL, "deconv3d: Wout must be 2 W, or 2 W minus the (at most 3) doubled padding columns"),
    ("Wout > 2 W", 1, 32, 32, 2, 4, 16, 34, 16, 16, 16, 16, 0, -EINVAL, "deconv3d: Wout must be 2 W, or 2 W minus the (at most 3) doubled padding columns"),
    ("Wout = 2 W - 8", 1, 32, 32, 2, 4, 16, 24, 16, 16, 16, 16, 0, -EINVAL, "deconv3d: Wout must be 2 W, or 2 W minus the (at most 3) doubled padding columns"),
    ("2 GiB", 1, 32, 32, 64, 1024, 1024, 2048, 16, 16, 16, 16, 0, -EUNSUPPORTED, "deconv3d: 8 input channels of one batch item must stay below 2 GiB (32-bit buffer offsets)"),
    ("just below 2 GiB", 1, 32, 32, 64, 1024, 1020, 2040, 16, 16, 16, 16, 0, 0x301, ""),
    ("Co 48", 2, 32, 48, 8, 64, 64, 128, 16, 16, 16, 16, 0, -EUNSUPPORTED, "deconv3d: output channels must be <= 32 or 64"),
    ("Co 48 small (split-K)", 1, 32, 48, 2, 4, 16, 32, 16, 16, 16, 16, 0, 0x100, ""),
    ("Co 128", 1, 32, 128, 2, 4, 16, 32, 16, 16, 16, 16, 0, -EUNSUPPORTED, "deconv3d: output channels must be <= 32 or 64"),
    ("queue grid too large", 4194304, 32, 32, 4, 64, 64, 128, 16, 16, 16, 16, 0, -EUNSUPPORTED, "deconv3d: grid too large"),
    ("ticket field: falls through", 524288, 32, 32, 4, 64, 64, 128, 16, 16, 16, 16, 0, 0x304, ""),
    ("ticket field: just fits", 524287, 32, 32, 4, 64, 64, 128, 16, 16, 16, 16, 0, 0x202, ""),
    ("two-parity grid too large", 16777216, 32, 32, 4, 64, 60, 120, 16, 16, 16, 0, 0, -EUNSUPPORTED, "deconv3d: grid too large"),
    ("output 2 GiB: no queue, no vepi", 1, 32, 64, 32, 512, 256, 512, 16, 16, 16, 16, 0, 0x306, ""),
    ("16 channels 2 GiB: no queue", 1, 32, 32, 32, 1024, 1024, 2048, 16, 16, 16, 16, 0, 0x301, ""),
]
REACHABLE = {0x100, 0x200, 0x201, 0x202, 0x204, 0x205, 0x206} | set(range(0x300, 0x30a))   # what the release library builds


def _plan(B, Ci, Co, D, H, W, Wout, xa=16, ya=16, ra=16, ws=16, sc=0):
    return _lib.load().dmb_deconv3d_k3s2_plan(B, Ci, Co, D, H, W, Wout, xa, ya, ra, ws, sc, NCU)


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_plan_is_the_recorded_one(case):
    lib = _lib.load()
    assert _plan(*case[1:13]) == case[13]
    assert lib.dmb_last_error().decode() == case[14]
    # without a device the library counts 256 compute units on its own
    assert lib.dmb_deconv3d_k3s2_plan(*case[1:13], 0) == case[13]


def test_recorded_cases_cover_every_instantiation_and_refusal():
    codes = {c[13] for c in CASES}
    assert codes - {-EINVAL, -EUNSUPPORTED} == REACHABLE
    assert {(c[13], c[14]) for c in CASES if c[13] < 0} == {
        (-EINVAL, "deconv3d: bad argument"),
        (-EINVAL, "deconv3d: Wout must be 2 W, or 2 W minus the (at most 3) doubled padding columns"),
        (-EUNSUPPORTED, "deconv3d: 8 input channels of one batch item must stay below 2 GiB (32-bit buffer offsets)"),
        (-EINVAL, "deconv3d: misaligned workspace"),
        (-EUNSUPPORTED, "deconv3d: grid too large"),
        (-EUNSUPPORTED, "deconv3d: a row-padded input (Wout < 2 W) needs the workspace form: Co 32 or 64, Ci % 16 == 0, Wout % 4 == 0, aligned operands"),
        (-EUNSUPPORTED, "deconv3d: output channels must be <= 32 or 64"),
    }


def _fake_cuda_tensor(shape, ptr=0x7f0000000000):
    return types.SimpleNamespace(shape=shape, is_cuda=True, data_ptr=lambda: ptr)


def test_width_sweep_names_built_tiles_only_and_padded_rows_agree():
    """W = 4, 8, ..., 2048 for both output widths, full rows and rows padded by one doubled column pair (Wout = 2 W - 4), small and
    large launches, with and without the single-chain flag and the workspace: no plan outside the instantiations the library builds
    -- in particular never the plain 60-column work-queue tile (tile 3), which the release build therefore leaves out -- and
    ops.padded_rows_applicable says yes exactly where the padded launch gets the work-queue form."""
    seen = set()
    for Co in (32, 64):
        for W in range(4, 2049, 4):
            for (B, D, H) in ((1, 1, 1), (1, 4, 6), (2, 12, 34), (4, 24, 68)):
                if 64 * 8 * D * H * W * 4 >= 2 ** 31 - 1:   # (the 2 GiB limits are in the table above)
                    continue
                for Wout in (2 * W, 2 * W - 4):
                    for sc in (0, 1):
                        for ws in (16, 0):
                            code = _plan(B, 64, Co, D, H, W, Wout, ws=ws, sc=sc)
                            assert code in REACHABLE or (code == -EUNSUPPORTED and Wout < 2 * W and ws == 0), (Co, W, B, D, H, Wout, sc, ws, code)
                            assert not (Wout < 2 * W and code >> 8 == ops.DECONV_PLAN_PARITY)
                            seen.add(code)
                # the unpadded tensor of a padded launch is 2 columns narrower than the multiple of 4
                for Ci in (64, 16):
                    x = _fake_cuda_tensor((B, Ci, D, H, W - 2))
                    want = _plan(B, Ci, Co, D, H, W, 2 * W - 4, sc=1) >> 8 == ops.DECONV_PLAN_QUEUE
                    assert ops.padded_rows_applicable(x, Co) == want == (Ci == 64), (Co, W, B, D, H, Ci)
    assert {c for c in REACHABLE if c >> 8 != ops.DECONV_PLAN_PARITY} <= seen   # every split-K and work-queue tile the library builds
    # what is truly Python's: a device tensor, W % 4 == 2; and x enters with its own alignment
    assert not ops.padded_rows_applicable(_fake_cuda_tensor((1, 64, 4, 6, 80)), 64)
    assert not ops.padded_rows_applicable(types.SimpleNamespace(shape=(1, 64, 4, 6, 78), is_cuda=False, data_ptr=lambda: 0), 64)
    assert ops.padded_rows_applicable(_fake_cuda_tensor((1, 64, 4, 6, 78)), 64)
    assert not ops.padded_rows_applicable(_fake_cuda_tensor((1, 64, 4, 6, 78), 0x7f0000000008), 64)
    assert not ops.padded_rows_applicable(_fake_cuda_tensor((1, 64, 4, 6, 78)), 48)
