"""CLI with --solver cpu-block (no GPU needed)."""

import numpy as np
import pytest

from acg_amd.gen import STENCIL_5PT_2D, stencil_global
from acg_amd.io.mtx import MtxFile, write_mtx
from acg_amd.utils.errors import AcgError


def _poisson_mtx(tmp_path, nx=12, ny=12):
    A = stencil_global(nx, ny, 1, STENCIL_5PT_2D)
    rows = np.repeat(np.arange(A.n), np.diff(A.rowptr))
    m = MtxFile(object="matrix", format="coordinate", field_="real",
                symmetry="symmetric", nrows=A.n, ncols=A.n,
                nnz=A.nnz_stored, rowidx=rows, colidx=A.colidx, a=A.vals)
    path = tmp_path / "A.mtx"
    write_mtx(path, m)
    return A, path


def _array_mtx(path, M):
    M = np.atleast_2d(M.T).T
    write_mtx(path, MtxFile(object="matrix", format="array", field_="real",
                            symmetry="general", nrows=M.shape[0],
                            ncols=M.shape[1], nnz=M.size,
                            a=np.ascontiguousarray(M.T).reshape(-1)))
    return path


def _run(monkeypatch, capsys, argv):
    from acg_amd import cli

    monkeypatch.delenv("WORLD_SIZE", raising=False)
    monkeypatch.delenv("RANK", raising=False)
    rc = cli.main([str(a) for a in argv])
    return rc, capsys.readouterr()


def _parse_array(text):
    lines = text.strip().splitlines()
    assert lines[0].startswith("%%MatrixMarket matrix array real general")
    nrows, ncols = (int(v) for v in lines[1].split())
    vals = np.array([float(v) for v in lines[2:]])
    assert len(vals) == nrows * ncols
    return vals.reshape(ncols, nrows).T


def _args(solver):
    return ["--solver", solver, "--max-iterations", "2000",
            "--residual-rtol", "1e-11"]


def test_cpu_block_b_file_matches_cpu(tmp_path, monkeypatch, capsys):
    A, path = _poisson_mtx(tmp_path)
    Xs = np.random.default_rng(3).standard_normal((A.n, 3))
    Bm = np.column_stack([A.dsymv(Xs[:, c].copy()) for c in range(3)])
    bpath = _array_mtx(tmp_path / "b.mtx", Bm)
    outs = {}
    for solver in ("cpu-block", "cpu"):
        rc, out = _run(monkeypatch, capsys, [path, bpath] + _args(solver))
        assert rc == 0, out.err
        outs[solver] = _parse_array(out.out)
        assert out.err.count("true residual") == 3
        for c in range(3):
            assert f"right-hand side {c}: true residual" in out.err
        assert out.err.count("solver: cg-block" if solver == "cpu-block"
                             else "solver: cg-cpu") == 3
    np.testing.assert_allclose(outs["cpu-block"], outs["cpu"], rtol=1e-6, atol=1e-8)
    np.testing.assert_allclose(outs["cpu-block"], Xs, rtol=1e-7, atol=1e-8)


def test_cpu_block_nrhs_matches_cpu(tmp_path, monkeypatch, capsys):
    A, path = _poisson_mtx(tmp_path)
    outs = {}
    for solver in ("cpu-block", "cpu"):
        rc, out = _run(monkeypatch, capsys, [path, "--nrhs", "3"] + _args(solver))
        assert rc == 0, out.err
        outs[solver] = _parse_array(out.out)
    assert outs["cpu-block"].shape == (A.n, 3)
    np.testing.assert_allclose(outs["cpu-block"], outs["cpu"], rtol=1e-6, atol=1e-8)


def test_cpu_block_one_rhs_is_cpu(tmp_path, monkeypatch, capsys):
    A, path = _poisson_mtx(tmp_path)
    rc, blk = _run(monkeypatch, capsys, [path] + _args("cpu-block"))
    assert rc == 0, blk.err
    rc, cpu = _run(monkeypatch, capsys, [path] + _args("cpu"))
    assert rc == 0
    assert blk.out == cpu.out and "solver: cg-cpu" in blk.err


def test_cpu_block_reports_the_handover(tmp_path, monkeypatch, capsys):
    A, path = _poisson_mtx(tmp_path)
    v = np.random.default_rng(5).standard_normal(A.n)
    bpath = _array_mtx(tmp_path / "b.mtx", np.column_stack([v, 4.0 * v]))
    rc, out = _run(monkeypatch, capsys, [path, bpath, "-v"] + _args("cpu-block"))
    assert rc == 0, out.err
    assert out.err.count("handed over to the per-column iteration at block "
                         "iteration 0") == 2
    X = _parse_array(out.out)
    np.testing.assert_allclose(X[:, 1], 4.0 * X[:, 0], rtol=1e-6, atol=1e-8)
    rc, quiet = _run(monkeypatch, capsys, [path, bpath] + _args("cpu-block"))
    assert rc == 0 and "handed over" not in quiet.err


def test_block_solvers_reject_diff_tolerances(tmp_path, monkeypatch, capsys):
    A, path = _poisson_mtx(tmp_path)
    for solver in ("cpu-block", "acg-block"):
        with pytest.raises(AcgError, match="diff"):
            _run(monkeypatch, capsys, [path, "--nrhs", "2", "--solver", solver,
                                       "--diff-rtol", "1e-3"])
