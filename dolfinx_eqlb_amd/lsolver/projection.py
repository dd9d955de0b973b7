"""Cell-local L2 projection into DG spaces on the GPU - mirror of
python/dolfinx_eqlb/lsolver/projection.py:17-77 (`local_projection`) on flat arrays.

The reference takes UFL expressions and JIT-compiles the load kernels; here the data are Python
callables f(x, y) -> array [..., bs] (or [...] for bs = 1) evaluated at the physical quadrature
points, or precomputed point values.
"""

import dataclasses
import typing

import numpy as np

from ..elmtlib.quadrature import make_quadrature_triangle
from ..eqlb.check_eqlb_conditions import cell_geometry


def quadrature_points_physical(mesh, qpoints):
    """x_c(X_q) for all cells: [ncells, nq, 2]."""
    J, _, _ = cell_geometry(mesh)
    x0 = mesh.x[mesh.cell_nodes[:, 0], :2]
    return x0[:, None, :] + np.einsum("cij,qj->cqi", J, qpoints)


@dataclasses.dataclass
class PrimalFlux:
    """sigma_h = -coeff grad(u_h) of a conforming P_p solution as an entry of `data` of local_projection: u [ndofs],
    cell_dofs [ncells, (p+1)(p+2)/2] (DOF transformations applied), coeff [ncells] or None.  Formed on the device
    from the solution vector (cpp.primal_flux_dg), without quadrature.  With cell_D [ncells, 3] = (d00, d01, d11) the
    flux is -coeff D grad(u_h), the one of PrimalPoisson.set_diffusion; a DG_0 tensor crosses a refinement through
    Refinement.prolong_dg(0, cell_D.ravel(), bs=3)."""
    u: typing.Any
    cell_dofs: typing.Any
    p: int
    coeff: typing.Any = None
    cell_D: typing.Any = None


@dataclasses.dataclass
class PrimalStress:
    """Row `row` (0 or 1) of sigma_h = -mu (2 eps(u_h) + pi_1 div(u_h) I) of a displacement u [ndofs, 2] in P_p^2 as an
    entry of `data` of local_projection (cpp.primal_stress_dg); pi_1 a number or an array [ncells].  The shear modulus
    is mu > 0 everywhere, or cell_mu [ncells] where given; a DG_0 cell_mu crosses a refinement through
    Refinement.prolong_dg(0, cell_mu).  The defaults give the non-dimensional stress (mu = 1)."""
    u: typing.Any
    cell_dofs: typing.Any
    p: int
    pi_1: typing.Any
    row: int
    mu: float = 1.0
    cell_mu: typing.Any = None


@dataclasses.dataclass
class PrimalValue:
    """coeff Pi_d u_h of a conforming P_p function as an entry of `data` of local_projection (bs = 1): u [ndofs],
    cell_dofs [ncells, (p+1)(p+2)/2], coeff [ncells] or None (no multiplication).  Formed on the device from the vector
    (cpp.primal_value_dg), without quadrature: with coeff = c_T the reaction part of the right-hand side an
    equilibrator needs (rhs = Pi_d f - c_T Pi_d u_h), with coeff = 1 / tau the u_old / tau of an implicit time step."""
    p: int
    cell_dofs: typing.Any
    u: typing.Any
    coeff: typing.Any = None


def _device_mesh(dmesh):
    """The cpp.DeviceMesh behind `dmesh` (made once per flat mesh container and kept on it)."""
    from .. import cpp
    if isinstance(dmesh, cpp.DeviceMesh):
        return dmesh
    cached = getattr(dmesh, "_cpp_device_mesh", None)
    if cached is None:
        cached = cpp.DeviceMesh(dmesh)
        try:
            dmesh._cpp_device_mesh = cached
        except AttributeError:
            pass
    return cached


def _check_primal(mesh, bs, d):
    ndp = (d.p + 1) * (d.p + 2) // 2
    stress = isinstance(d, PrimalStress)
    usize = np.size(d.u)
    if isinstance(d, PrimalValue):
        if bs != 1 or np.size(d.cell_dofs) != mesh.ncells * ndp or usize == 0:
            raise RuntimeError("Local solver: Input sizes does not match")
        return
    if (bs != 2 or np.size(d.cell_dofs) != mesh.ncells * ndp or usize == 0 or (stress and usize % 2)
            or (stress and d.row not in (0, 1))):
        raise RuntimeError("Local solver: Input sizes does not match")


def _project_primal(dmesh, degree, d):
    from .. import cpp
    dm = _device_mesh(dmesh)
    if isinstance(d, PrimalValue):
        return cpp.primal_value_dg(dm, d.p, degree, d.cell_dofs, np.asarray(d.u, dtype=np.float64).reshape(1, -1),
                                   d.coeff)[0]
    if isinstance(d, PrimalStress):
        per_cell = np.ndim(d.pi_1) > 0
        out = cpp.primal_stress_dg(dm, d.p, degree, d.cell_dofs, d.u, 1.0 if per_cell else float(d.pi_1),
                                   d.pi_1 if per_cell else None, mu=float(d.mu), cell_mu=d.cell_mu)
        return np.ascontiguousarray(out[d.row])
    return cpp.primal_flux_dg(dm, d.p, degree, d.cell_dofs, np.asarray(d.u, dtype=np.float64).reshape(1, -1),
                              d.coeff, cell_D=d.cell_D)[0]


def local_projection(dmesh, degree: int, data: typing.List[typing.Any], bs: int = 1,
                     quadrature_degree: typing.Optional[int] = None,
                     solver: str = "cholesky") -> typing.List[np.ndarray]:
    """Project every entry of `data` into DG_degree (block size bs); returns the DOF arrays
    [ncells*nd*bs] (cell-major, x[bs*dof+cb]).  data[i]: callable(x, y), array [ncells, nq, bs], a PrimalFlux /
    PrimalStress (bs = 2: the flux or a stress row of a P_p solution, formed on the device from its DOFs), or a
    PrimalValue (bs = 1: the projected value of a P_p function, times a cell-wise coefficient).
    `dmesh`: flat mesh container (or a `cpp.DeviceMesh` of one).  The solve runs through
    `local_solver_<solver>` of the compiled module (names of python/dolfinx_eqlb/wrappers.cpp:52-80):
    a = (u, v) on DG_degree, l_i = (f_i, v) given by the point values of f_i."""
    from ..eqlb import _adapter
    c = _adapter.module()
    mesh = getattr(dmesh, "mesh", dmesh)
    qdeg = 2 * degree + 2 if quadrature_degree is None else quadrature_degree
    qp, qw = make_quadrature_triangle(qdeg)
    xq = None
    is_primal = [isinstance(d, (PrimalFlux, PrimalStress, PrimalValue)) for d in data]
    for d, pr in zip(data, is_primal):
        if pr:
            _check_primal(mesh, bs, d)
    V = _adapter.dg_space(mesh, degree, bs) if not (data and all(is_primal)) else None
    sols, forms = [], []
    primal = {}
    for i, d in enumerate(data):
        if is_primal[i]:
            primal[i] = _project_primal(dmesh, degree, d)
            continue
        if callable(d):
            if xq is None:
                xq = quadrature_points_physical(mesh, qp)
            v = np.asarray(d(xq[..., 0], xq[..., 1]), dtype=np.float64)
        else:
            v = np.asarray(d, dtype=np.float64)
        if v.size != mesh.ncells * qw.size * bs:
            raise RuntimeError("Local solver: Input sizes does not match")
        forms.append(c.Form.from_point_values(qp, qw, np.ascontiguousarray(v.reshape(mesh.ncells, qw.size, bs))))
        sols.append(c.Function(V))
    fn = {"cholesky": c.local_solver_cholesky, "lu": c.local_solver_lu, "cg": c.local_solver_cg}[solver]
    if V is not None:
        fn(sols, c.Form([]), forms)
    rest = iter(s_.array for s_ in sols)
    return [primal[i] if i in primal else next(rest) for i in range(len(data))]


def embed_dg(values, ncells: int, degree_from: int, degree_to: int, bs: int = 1):
    """Exact embedding DG_{degree_from} -> DG_{degree_to} (degree_to >= degree_from) of nodal
    values [ncells*nd_from*bs]: the reference accepts projected data of any degree <= k-1
    (se/reconstruction.hpp:363-373).  The equilibrators and the estimator entry points (eqlb_se_estimate_dg,
    eqlb_ev_estimate_dg, eqlb_oscillation_dg, eqlb_boundary_residual) read it as it is; the embedding is what
    the tests compare them with."""
    import numpy as np

    from ..elmtlib.lagrange import Lagrange
    if degree_to < degree_from:
        raise RuntimeError("Equilibration: Wrong polynomial degree of the projected RHS")
    lo, hi = Lagrange(degree_from), Lagrange(degree_to)
    nodes = np.array([[float(a), float(b)] for a, b in hi.nodes])
    E = lo.tabulate(nodes)[0]  # [nd_to, nd_from]
    v = np.asarray(values, dtype=np.float64).reshape(ncells, lo.ndofs, bs)
    return np.ascontiguousarray(np.einsum("ij,cjb->cib", E, v).reshape(-1))
