"""World-2 gloo: shifted, reversed and transposed reads of an index-pure 2-D
array across the shard boundary are recomputed from the index
(common.remat), so they equal NumPy and the per-exchange byte counters show
that no halo bytes moved; with the switch off the same reads do exchange.

The input is not affine in the index and the stencil weights all differ, so
a wrong offset, step, axis order or per-rank global start in the composed
recipe changes the result."""

from test_distributed_gloo import run_spmd


def test_shifted_read_of_pure_array_moves_no_halo():
    run_spmd("""
        from ramba_amd import common

        def moved():
            return common.timing_acc.get("exchange_bytes", (0, 0.0))[1]

        def reads(X):
            st = (0.5 * X[:-2, 1:-1] + 2.0 * X[2:, 1:-1] + 3.0 * X[1:-1, :-2]
                  - 1.5 * X[1:-1, 2:] - 4.0 * X[1:-1, 1:-1])
            rev = X[::-1, ::2] - 2.0 * X[:, :35]
            tr = X.T[1:, 3:] + 1.0
            return st, rev, tr

        def host(parts):
            return np.concatenate(
                [(p.asarray() if hasattr(p, "asarray") else p).reshape(-1)
                 for p in parts])

        X = np_.fromfunction(lambda x, y: x * x + y * x, (66, 70),
                             dtype=np.float64)
        if np_ is np:
            ref = host(reads(X))
            assert np.any(ref != 0)
            return ref
        common.remat, common.remat_min_bytes = 1, 0
        np_.sync()
        b0, s0 = moved(), common.remat_substitutions
        R = reads(X)
        np_.sync()
        assert common.remat_substitutions - s0 >= 8, "reads not rematerialised"
        assert moved() == b0, f"halo bytes moved: {moved() - b0}"
        # control: the same reads from memory cross the shard boundary
        common.remat = 0
        R_off = reads(X)
        np_.sync()
        assert moved() > b0, "control run exchanged no halo"
        common.remat = 1
        on, off = host(R), host(R_off)
        assert np.array_equal(on, off)
        return on
    """, world=2)
