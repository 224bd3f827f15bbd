"""CLI with several right-hand sides, host solver (no GPU needed)."""

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
    """n x k array file, column-major as Matrix Market prescribes."""
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
    out = capsys.readouterr()
    return rc, out


def _parse_array(text):
    lines = text.strip().splitlines()
    assert lines[0].startswith("%%MatrixMarket matrix array real general")
    nrows, ncols = (int(v) for v in lines[1].split())
    vals = np.array([float(v) for v in lines[2:]])
    assert len(vals) == nrows * ncols
    return vals.reshape(ncols, nrows).T


ARGS = ["--solver", "cpu", "--max-iterations", "2000", "--residual-rtol", "1e-11"]


def test_multi_column_b_roundtrips(tmp_path, monkeypatch, capsys):
    A, path = _poisson_mtx(tmp_path)
    rng = np.random.default_rng(3)
    Xs = rng.standard_normal((A.n, 3))
    Bm = np.column_stack([A.dsymv(Xs[:, c].copy()) for c in range(3)])
    bpath = _array_mtx(tmp_path / "b.mtx", Bm)
    rc, out = _run(monkeypatch, capsys, [path, bpath] + ARGS)
    assert rc == 0, out.err
    X = _parse_array(out.out)
    assert X.shape == (A.n, 3)
    np.testing.assert_allclose(X, Xs, rtol=1e-7, atol=1e-8)
    for c in range(3):
        assert f"right-hand side {c}: true residual" in out.err
    # each column is what a single-RHS run of that column gives
    b1 = _array_mtx(tmp_path / "b1.mtx", Bm[:, 1])
    rc, out1 = _run(monkeypatch, capsys, [path, b1] + ARGS)
    assert rc == 0
    assert np.array_equal(_parse_array(out1.out)[:, 0], X[:, 1])


def test_multi_column_x0(tmp_path, monkeypatch, capsys):
    A, path = _poisson_mtx(tmp_path)
    rng = np.random.default_rng(4)
    Xs = rng.standard_normal((A.n, 2))
    Bm = np.column_stack([A.dsymv(Xs[:, c].copy()) for c in range(2)])
    bpath = _array_mtx(tmp_path / "b.mtx", Bm)
    # the exact solution as initial guess: converged at iteration 0
    rc, out = _run(monkeypatch, capsys,
                   [path, bpath, _array_mtx(tmp_path / "x0.mtx", Xs)] + ARGS)
    assert rc == 0, out.err
    assert out.err.count("iterations: 0 ") == 2
    # (the text reader is within a few 1e-16 of the written value)
    np.testing.assert_allclose(_parse_array(out.out), Xs, rtol=1e-13, atol=1e-15)
    # x0 of another shape is refused
    x1 = _array_mtx(tmp_path / "x1.mtx", Xs[:, 0])
    with pytest.raises(AcgError, match="x0 has shape"):
        _run(monkeypatch, capsys, [path, bpath, x1] + ARGS)
    x3 = _array_mtx(tmp_path / "x3.mtx", np.column_stack([Xs, Xs[:, 0]]))
    with pytest.raises(AcgError, match="x0 has shape"):
        _run(monkeypatch, capsys, [path, bpath, x3] + ARGS)


@pytest.mark.parametrize("extra", [[], ["--manufactured-solution", "--seed", "7"]])
def test_nrhs_column0_is_the_single_rhs_output(tmp_path, monkeypatch, capsys, extra):
    A, path = _poisson_mtx(tmp_path)
    rc, single = _run(monkeypatch, capsys, [path] + ARGS + extra)
    assert rc == 0
    rc, multi = _run(monkeypatch, capsys, [path, "--nrhs", "3"] + ARGS + extra)
    assert rc == 0, multi.err
    s_lines = single.out.strip().splitlines()
    m_lines = multi.out.strip().splitlines()
    assert m_lines[1].split() == [str(A.n), "3"]
    assert len(m_lines) == 2 + 3 * A.n
    # column-major: column 0 comes first, byte for byte the single output
    assert m_lines[2:2 + A.n] == s_lines[2:]
    X = _parse_array(multi.out)
    assert not np.array_equal(X[:, 1], X[:, 0]) and not np.array_equal(X[:, 2], X[:, 1])
    if extra:
        assert multi.err.count("manufactured solution: ||x-x*||") == 3
        # column c > 0: x* drawn from default_rng(seed + c), normalised
        for c in (1, 2):
            xs = np.random.default_rng(7 + c).standard_normal(A.n)
            xs /= np.linalg.norm(xs)
            np.testing.assert_allclose(X[:, c], xs, rtol=1e-6, atol=1e-8)
    else:
        for c in (1, 2):
            b = np.random.default_rng(c).standard_normal(A.n)
            np.testing.assert_allclose(A.dsymv(X[:, c].copy()), b, rtol=1e-6, atol=1e-8)


def test_single_rhs_output_has_no_column_labels(tmp_path, monkeypatch, capsys):
    A, path = _poisson_mtx(tmp_path)
    rc, out = _run(monkeypatch, capsys, [path, "--nrhs", "1"] + ARGS)
    assert rc == 0
    assert "right-hand side" not in out.err
    assert out.out.strip().splitlines()[1].split() == [str(A.n), "1"]


def test_multi_rhs_refused_by_other_solvers(tmp_path, monkeypatch, capsys):
    A, path = _poisson_mtx(tmp_path)
    for solver in ("acg-pipelined", "cpu-pipelined", "scipy", "acg-mixed"):
        with pytest.raises(AcgError, match="right-hand sides are not supported"):
            _run(monkeypatch, capsys, [path, "--nrhs", "2", "--solver", solver])
    bpath = _array_mtx(tmp_path / "b.mtx", np.ones((A.n, 2)))
    with pytest.raises(AcgError, match="right-hand sides are not supported"):
        _run(monkeypatch, capsys, [path, bpath, "--solver", "cpu-pipelined"])
    with pytest.raises(AcgError, match="cannot be combined with a b file"):
        _run(monkeypatch, capsys, [path, bpath, "--nrhs", "2", "--solver", "cpu"])
    with pytest.raises(AcgError, match="diff"):
        _run(monkeypatch, capsys, [path, "--nrhs", "2", "--solver", "cpu",
                                   "--diff-rtol", "1e-3"])
