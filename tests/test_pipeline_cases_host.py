"""The inputs of the pipeline edge tests hold what those tests lean on; the
conditions are asserted when pipeline_cases is imported, so this runs them on
a machine without a GPU."""
import numpy as np

import pipeline_cases as PC


def test_the_conditions_of_the_inputs_hold():
    PC._check_inputs()
    assert set(PC.READS) == set(PC.RICH) | {"dense"}
    assert sorted(PC.length_of(n) for n in PC.RICH) == [32, 33, 48, 100]


def test_expected_lists_are_shared_and_read_only():
    a = PC.expected("m32", PC.MUMCAND, 0, 100)
    assert PC.expected("m32", PC.MUMCAND, 0, 100) is a
    assert not a.flags.writeable
    sizes = [40, 0, 60]
    parts = PC.per_batch(a, sizes)
    assert [len(x) for x in parts] == PC.batch_counts(a, sizes)
    assert np.array_equal(PC.joined(parts), a)
