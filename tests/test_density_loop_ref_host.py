"""CPU: the reference controller (density_ref.ReferenceController, CTRL:130-168 around CTRL:170-353) in a closed loop with the
oracle's forward / backward and torch.optim.Adam, on the inputs of density_loop_case.py.  No device code runs here: the test
fixes the inputs of tests/test_gpu_density_loop.py and shows, on the reference's own counts, that they reach every branch the
device is then compared in."""
import density_loop_case as L


def test_the_loop_reaches_every_branch():
    cycles, resets, moved_share = L.run_reference_loop()
    print(L.counts_table(cycles))
    print("alpha resets (iteration, on a densify iteration, rows lowered):", resets, " moved sources:", moved_share)
    assert [c["iteration"] for c in cycles] == [2, 4, 6, 8, 10, 12]
    assert [r[:2] for r in resets] == [(5, False), (10, True)]
    assert all(rows_lowered >= 100 for _, _, rows_lowered in resets)         # neither reset is a no-op
    L.assert_branch_conditions(cycles, resets, moved_share, L.controller_config())
