"""Out-of-bounds audit of csrc/segment_rows.hip: the operator tests of tests/test_gpu_pointnet.py (the four kernels at the
tile and chunk seams, every k, row strides, the odd widths) again in a process whose every device allocation ends at the
end of its own mapping (tests/guard/run_guarded.py, as tests/test_gpu_guard.py uses it).  The memory-peak test is left
out: a pluggable allocator keeps no statistics.  The reference compositions of those tests gather with `index_select`:
the backward of `T[batch]` is ATen's indexing_backward_kernel_small_stride, which reads past the end of its index buffer
on this ROCm build ("The intermittent abort") and ends a guarded process."""
import os
import subprocess
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.mark.gpu
def test_segment_row_kernels_under_the_guard_allocator():
    sel = ["tests/test_gpu_pointnet.py", "-m", "gpu", "-k",
           "segment_transform_distance or identity_matrices or segment_broadcast_cat or segment_mean_rows"]
    out = subprocess.run([sys.executable, os.path.join(HERE, "guard", "run_guarded.py")] + sel, env=dict(os.environ),
                         stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    marks = [l for l in out.stdout.splitlines() if "Fatal" in l or "fault" in l or "test_gpu_pointnet.py" in l][-12:]
    tail = "\n".join(marks) + "\n...\n" + out.stdout[-3000:]
    assert "Memory access fault" not in out.stdout, tail
    assert out.returncode == 0, tail
    assert " passed" in out.stdout and "no tests ran" not in out.stdout, tail
