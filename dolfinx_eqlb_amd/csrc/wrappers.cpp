// pybind11 module `dolfinx_eqlb_amd._cpp`: the names, argument order and error behaviour of the
// reference's binding `dolfinx_eqlb.cpp` (python/dolfinx_eqlb/wrappers.cpp:52-272) over the C ABI of
// libeqlb_amd.so (include/eqlb.h).
//
//   reference (DOLFINx objects)                          here
//   ------------------------------------------------    -------------------------------------------------
//   dolfinx::mesh::Mesh                                  Mesh(x, cell_nodes, ..., facet_perm)  flat arrays
//   dolfinx::fem::FunctionSpace                          FunctionSpace(mesh, family, degree, bs, discontinuous)
//   dolfinx::fem::Function<double>                       Function(V[, array]) / Function.from_device(V, ptr)
//   dolfinx::fem::Constant<double>                       Constant(values)
//   dolfinx::fem::Form<double>                           Form(coefficients) / Form.from_point_values(...)
//   FluxBC(function_space, facets, pointer_boundary_kernel, nevals_per_fct[, quadrature_degree],
//          coefficients, position_of_coefficients, constants)              wrappers.cpp:144-232  same
//   BoundaryData(list_of_bcs, list_of_boundary_fluxes, V_flux_hdiv, rtflux_is_custom, quadrature_degree,
//                list_bfcts_prime, reconstruct_stress)                     wrappers.cpp:235-256  same
//   reconstruct_fluxes_semiexplt[_with_kornconst], reconstruct_fluxes_minimisation,
//   local_solver_lu / _cholesky / _cg                                      wrappers.cpp:52-137   same
//
// `pointer_boundary_kernel` is the address of a function with the signature of
// ufcx_expression::tabulate_tensor_float64 (the reference passes the ufcx_expression and takes that
// member, wrappers.cpp:164-172; FFCx' header is not part of this build).  The DOLFINx-object overloads
// (zero-copy from Function.x.array) belong in dolfinx_adapter.h, compiled only where <dolfinx/...> exists.
// C++ exceptions (std::runtime_error) arrive in Python as RuntimeError, as in the reference.
#include <pybind11/numpy.h>
#include <pybind11/pybind11.h>
#include <pybind11/stl.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <map>
#include <memory>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../include/eqlb.h"

namespace py = pybind11;

namespace
{
using darray = py::array_t<double, py::array::c_style | py::array::forcecast>;
template <typename T>
using carray = py::array_t<T, py::array::c_style | py::array::forcecast>;

// an optional array argument: the array, kept alive, and its data - nullptr for None.  One of another size than n
// throws `what`
struct OptArray
{
  carray<double> a;
  const double* p = nullptr;
};
OptArray opt_array(const py::object& o, py::ssize_t n, const std::string& what)
{
  OptArray r;
  if (!o.is_none())
  {
    r.a = o.cast<carray<double>>();
    if (r.a.size() != n)
      throw std::runtime_error(what);
    r.p = r.a.data();
  }
  return r;
}

[[noreturn]] void raise_last(int status)
{
  const char* msg = eqlb_last_error();
  throw std::runtime_error((msg && *msg) ? std::string(msg) : "eqlb error " + std::to_string(status));
}
inline void check(int status)
{
  if (status != EQLB_OK)
    raise_last(status);
}

void* g_stream = nullptr; // hipStream_t of device-memory calls (set_stream)

// ---- stand-ins of the DOLFINx objects -------------------------------------------------------------
struct Transfer;

struct Mesh
{
  eqlb_mesh_t* h = nullptr;
  int32_t nnodes = 0, ncells = 0, nfacets = 0;
  std::vector<double> x;
  std::vector<int32_t> cell_nodes, cell_facets, facet_nodes, facet_cells_off, facet_cells;
  std::vector<uint8_t> facet_perm;

  Mesh(carray<double> x_, carray<int32_t> cn, carray<int32_t> cf, carray<int32_t> fn, carray<int32_t> fco,
       carray<int32_t> fc, carray<int32_t> nco, carray<int32_t> nc, carray<int32_t> nfo, carray<int32_t> nf,
       carray<uint8_t> fp)
  {
    if (x_.ndim() != 2 || x_.shape(1) != 3 || cn.ndim() != 2 || cn.shape(1) != 3 || fn.ndim() != 2)
      throw std::runtime_error("Mesh: x [nnodes, 3], cell_nodes [ncells, 3], facet_nodes [nfacets, 2] expected");
    nnodes = (int32_t)x_.shape(0);
    ncells = (int32_t)cn.shape(0);
    nfacets = (int32_t)fn.shape(0);
    if (cf.size() != (py::ssize_t)ncells * 3 || fp.size() != (py::ssize_t)ncells * 3 || fco.size() != nfacets + 1
        || nco.size() != nnodes + 1 || nfo.size() != nnodes + 1)
      throw std::runtime_error("Mesh: inconsistent array sizes");
    x.assign(x_.data(), x_.data() + x_.size());
    cell_nodes.assign(cn.data(), cn.data() + cn.size());
    cell_facets.assign(cf.data(), cf.data() + cf.size());
    facet_nodes.assign(fn.data(), fn.data() + fn.size());
    facet_cells_off.assign(fco.data(), fco.data() + fco.size());
    facet_cells.assign(fc.data(), fc.data() + fc.size());
    facet_perm.assign(fp.data(), fp.data() + fp.size());
    check(eqlb_mesh_create(nnodes, ncells, nfacets, x.data(), cell_nodes.data(), cell_facets.data(),
                           facet_nodes.data(), fco.data(), fc.data(), nco.data(), nc.data(), nfo.data(),
                           nf.data(), fp.data(), &h));
  }
  ~Mesh() { eqlb_mesh_destroy(h); }
  Mesh(const Mesh&) = delete;
  Mesh& operator=(const Mesh&) = delete;

  // the topology derived on the device (eqlb_mesh_create_from_cells); the host vectors come from the export
  static std::shared_ptr<Mesh> from_cells(carray<double> x_, carray<int32_t> cn)
  {
    if (x_.ndim() != 2 || (x_.shape(1) != 2 && x_.shape(1) != 3) || cn.ndim() != 2 || cn.shape(1) != 3)
      throw std::runtime_error("Mesh.from_cells: x [nnodes, 2 or 3], cell_nodes [ncells, 3] expected");
    std::shared_ptr<Mesh> m(new Mesh());
    m->nnodes = (int32_t)x_.shape(0);
    m->ncells = (int32_t)cn.shape(0);
    const int gdim = (int)x_.shape(1);
    m->x.assign(3 * (size_t)m->nnodes, 0.0);
    for (size_t i = 0; i < (size_t)m->nnodes; ++i)
      for (int j = 0; j < gdim; ++j)
        m->x[3 * i + j] = x_.data()[gdim * i + j];
    m->cell_nodes.assign(cn.data(), cn.data() + cn.size());
    check(eqlb_mesh_create_from_cells(m->nnodes, m->ncells, m->x.data(), m->cell_nodes.data(), EQLB_MEM_HOST, nullptr,
                                      &m->h));
    m->export_tables();
    return m;
  }

  // the mesh refined at the cells `marked` on the device (eqlb_mesh_refine_plan ...): the new Mesh, parent_cell,
  // node_parent_facet, parent_facet; with keep_plan a Transfer (below) as fifth entry, which carries host arrays over
  static py::tuple refine(std::shared_ptr<Mesh> self, carray<int32_t> marked, bool keep_plan);

  // (cell_dofs [ncells, nd_p], ndofs) of the conforming P_p space (eqlb_mesh_lagrange_dofmap)
  py::tuple lagrange_dofmap(int p) const
  {
    if (p < 1 || p > 4)
      throw std::runtime_error("Mesh.lagrange_dofmap: p outside 1 ... 4");
    py::array_t<int32_t> cd({(py::ssize_t)ncells, (py::ssize_t)((p + 1) * (p + 2) / 2)});
    int64_t ndofs = 0;
    check(eqlb_mesh_lagrange_dofmap(h, p, cd.mutable_data(), &ndofs, EQLB_MEM_HOST, nullptr));
    return py::make_tuple(cd, ndofs);
  }

  py::array_t<int32_t> boundary_facets() const
  {
    int32_t n = 0;
    std::vector<int32_t> all((size_t)nfacets);
    check(eqlb_mesh_boundary_facets(h, all.data(), nfacets, &n, EQLB_MEM_HOST, nullptr));
    return py::array_t<int32_t>(n, all.data());
  }

  py::array_t<int32_t> find_facets(carray<int32_t> pairs) const
  {
    if (pairs.size() % 2 != 0)
      throw std::runtime_error("Mesh.find_facets: pairs [npairs, 2] expected");
    const int32_t np_ = (int32_t)(pairs.size() / 2);
    py::array_t<int32_t> out(np_);
    check(eqlb_mesh_find_facets(h, np_, pairs.data(), out.mutable_data(), EQLB_MEM_HOST, nullptr));
    return out;
  }

private:
  Mesh() = default;

  // nfacets and the host tables of a handle built on the device
  void export_tables()
  {
    check(eqlb_mesh_counts(h, nullptr, nullptr, &nfacets));
    cell_facets.resize(3 * (size_t)ncells);
    facet_nodes.resize(2 * (size_t)nfacets);
    facet_cells_off.resize((size_t)nfacets + 1);
    facet_cells.resize(3 * (size_t)ncells);
    facet_perm.resize(3 * (size_t)ncells);
    check(eqlb_mesh_export(h, cell_facets.data(), facet_nodes.data(), facet_cells_off.data(), facet_cells.data(),
                           nullptr, nullptr, nullptr, nullptr, facet_perm.data(), EQLB_MEM_HOST, nullptr));
  }

public:

  // affine map of a cell: J (dx_i/dX_j), detJ
  double jacobian(int32_t c, double J[2][2]) const
  {
    const int32_t* v = &cell_nodes[3 * (size_t)c];
    for (int i = 0; i < 2; ++i)
    {
      J[i][0] = x[3 * (size_t)v[1] + i] - x[3 * (size_t)v[0] + i];
      J[i][1] = x[3 * (size_t)v[2] + i] - x[3 * (size_t)v[0] + i];
    }
    return J[0][0] * J[1][1] - J[0][1] * J[1][0];
  }
};

// The open plan of a refinement with the two meshes it connects: prolongation of host arrays
// (eqlb_refine_prolong_lagrange, eqlb_refine_prolong_dg)
struct Transfer
{
  eqlb_refine_t* plan = nullptr;
  std::shared_ptr<Mesh> coarse, fine; // the plan reads the old handle: both stay alive with the carrier
  ~Transfer() { eqlb_refine_destroy(plan); }
  Transfer() = default;
  Transfer(const Transfer&) = delete;
  Transfer& operator=(const Transfer&) = delete;

  // u [nrhs, ndofs*bs] or [ndofs*bs] -> [nrhs, ndofs2*bs]; dofmaps None: lagrange_dofmap of the two meshes
  darray prolong(int p, darray u, py::object cell_dofs, py::object cell_dofs2, int bs, py::object ndofs2_) const
  {
    if (p < 1 || p > 4 || bs < 1)
      throw std::runtime_error("Transfer.prolong: p outside 1 ... 4 or bs < 1");
    const int nd = (p + 1) * (p + 2) / 2;
    const py::ssize_t nrhs = u.ndim() == 2 ? u.shape(0) : 1, nu = u.size() / nrhs;
    int64_t ndofs2 = 0;
    carray<int32_t> cd = cell_dofs.is_none() ? coarse->lagrange_dofmap(p)[0].cast<carray<int32_t>>()
                                             : cell_dofs.cast<carray<int32_t>>();
    carray<int32_t> cd2;
    if (cell_dofs2.is_none())
    {
      py::tuple t = fine->lagrange_dofmap(p);
      cd2 = t[0].cast<carray<int32_t>>();
      ndofs2 = t[1].cast<int64_t>();
    }
    else
    {
      cd2 = cell_dofs2.cast<carray<int32_t>>();
      for (py::ssize_t i = 0; i < cd2.size(); ++i)
        ndofs2 = std::max<int64_t>(ndofs2, (int64_t)cd2.data()[i] + 1);
    }
    if (!ndofs2_.is_none())
      ndofs2 = ndofs2_.cast<int64_t>();
    if (nu % bs != 0 || cd.size() != (py::ssize_t)coarse->ncells * nd || cd2.size() != (py::ssize_t)fine->ncells * nd)
      throw std::runtime_error("Transfer.prolong: Input sizes does not match");
    darray out({nrhs, (py::ssize_t)(ndofs2 * bs)});
    std::fill(out.mutable_data(), out.mutable_data() + out.size(), 0.0);
    check(eqlb_refine_prolong_lagrange(plan, fine->h, p, bs, (int32_t)nrhs, cd.data(), nu / bs, u.data(), cd2.data(),
                                       ndofs2, out.mutable_data(), EQLB_MEM_HOST, nullptr));
    return out;
  }

  // values [nrhs, ncells*nd*bs] or 1-D -> [nrhs, ncells2*nd*bs]
  darray prolong_dg(int degree, darray values, int bs) const
  {
    if (degree < 0 || degree > 3 || bs < 1)
      throw std::runtime_error("Transfer.prolong_dg: degree outside 0 ... 3 or bs < 1");
    const py::ssize_t row = (py::ssize_t)((degree + 1) * (degree + 2) / 2) * bs;
    const py::ssize_t nrhs = values.ndim() == 2 ? values.shape(0) : 1;
    if (values.size() != nrhs * coarse->ncells * row)
      throw std::runtime_error("Transfer.prolong_dg: Input sizes does not match");
    darray out({nrhs, (py::ssize_t)fine->ncells * row});
    check(eqlb_refine_prolong_dg(plan, fine->h, degree, bs, (int32_t)nrhs, values.data(), out.mutable_data(),
                                 EQLB_MEM_HOST, nullptr));
    return out;
  }

  // facet_type [nrhs, nfacets] or 1-D -> [nrhs, nfacets2] (eqlb_refine_facet_types)
  py::array_t<int8_t> facet_types(carray<int8_t> facet_type) const
  {
    const py::ssize_t nrhs = facet_type.ndim() == 2 ? facet_type.shape(0) : 1;
    if (facet_type.size() != nrhs * coarse->nfacets)
      throw std::runtime_error("Transfer.facet_types: Input sizes does not match");
    py::array_t<int8_t> out({nrhs, (py::ssize_t)fine->nfacets});
    check(eqlb_refine_facet_types(plan, fine->h, (int32_t)nrhs, facet_type.data(), out.mutable_data(), EQLB_MEM_HOST,
                                  nullptr));
    return out;
  }

  // old facet ids [nlist] -> children [nlist, 2] in the numbering of the refined mesh (eqlb_refine_child_facets)
  py::array_t<int32_t> child_facets(carray<int32_t> facets) const
  {
    const py::ssize_t nlist = facets.size();
    py::array_t<int32_t> out({nlist, (py::ssize_t)2});
    check(eqlb_refine_child_facets(plan, fine->h, (int32_t)nlist, facets.data(), out.mutable_data(), EQLB_MEM_HOST,
                                   nullptr));
    return out;
  }

  // boundary_values [nrhs, ncells*k(k+2)] or 1-D -> dofs [nrhs, nlist, k] of the boundary facets facets2 of the
  // refined mesh (eqlb_refine_prolong_flux_bc)
  darray prolong_flux_bc(int k, darray boundary_values, carray<int32_t> facets2) const
  {
    if (k < 1 || k > 4)
      throw std::runtime_error("Transfer.prolong_flux_bc: k outside 1 ... 4");
    const py::ssize_t nrhs = boundary_values.ndim() == 2 ? boundary_values.shape(0) : 1, nlist = facets2.size();
    if (boundary_values.size() != nrhs * coarse->ncells * k * (k + 2))
      throw std::runtime_error("Transfer.prolong_flux_bc: Input sizes does not match");
    darray out({nrhs, nlist, (py::ssize_t)k});
    check(eqlb_refine_prolong_flux_bc(plan, fine->h, k, (int32_t)nrhs, boundary_values.data(), (int32_t)nlist,
                                      facets2.data(), out.mutable_data(), EQLB_MEM_HOST, nullptr));
    return out;
  }
};

// several right-hand sides: the column count of an array [nrhs][n], and the list of the columns' info dicts
static int32_t many_columns(const darray& a, int64_t n, const char* who)
{
  if (a.ndim() != 2 || a.shape(0) < 1 || a.shape(1) != n)
    throw std::runtime_error(std::string(who) + ": Input sizes does not match");
  return (int32_t)a.shape(0);
}
static py::list many_info(const std::vector<double>& v)
{
  py::list out;
  for (size_t c = 0; c + 8 <= v.size(); c += 8)
  {
    py::dict info;
    info["iterations"] = (int64_t)v[c];
    info["converged"] = (int64_t)v[c + 1];
    info["nb"] = v[c + 2];
    info["rnorm"] = v[c + 3];
    info["replacements"] = (int64_t)v[c + 4];
    info["breakdown"] = (int64_t)v[c + 5];
    info["tol"] = v[c + 6];
    info["facets_skipped"] = (int64_t)v[c + 7];
    out.append(info);
  }
  return out;
}

// (indptr int64 [n + 1], indices int32 [nnz], values [nnz]) of a solver handle as CSR, on host arrays: `pattern`,
// `exp` and `vals` are the eqlb_*_matrix_* entries of the handle type
template <class H, class Pattern, class Export, class Values>
py::tuple matrix_of(H* h, int64_t rows, bool eliminate, Pattern pattern, Export exp, Values vals)
{
  int64_t nnz = 0;
  check(pattern(h, &nnz, nullptr));
  py::array_t<int64_t> indptr((py::ssize_t)(rows + 1));
  py::array_t<int32_t> indices((py::ssize_t)nnz);
  darray values((py::ssize_t)nnz);
  check(exp(h, indptr.mutable_data(), indices.mutable_data(), EQLB_MEM_HOST, nullptr));
  check(vals(h, eliminate ? 1 : 0, values.mutable_data(), nnz, EQLB_MEM_HOST, nullptr));
  return py::make_tuple(indptr, indices, values);
}
template <class H, class Pattern, class Values>
darray matrix_values_of(H* h, bool eliminate, Pattern pattern, Values vals)
{
  int64_t nnz = 0;
  check(pattern(h, &nnz, nullptr));
  darray values((py::ssize_t)nnz);
  check(vals(h, eliminate ? 1 : 0, values.mutable_data(), nnz, EQLB_MEM_HOST, nullptr));
  return values;
}

// y = A x for a CSR matrix, on the device (eqlb_csr_apply), on host arrays
darray csr_apply(carray<int64_t> indptr, carray<int32_t> indices, carray<double> values, carray<double> x)
{
  if (indptr.size() != x.size() + 1 || indices.size() != values.size())
    throw std::runtime_error("csr_apply: Input sizes does not match");
  darray y((py::ssize_t)x.size());
  check(eqlb_csr_apply((int64_t)x.size(), indptr.data(), indices.data(), values.data(), x.data(), y.mutable_data(),
                       EQLB_MEM_HOST, nullptr));
  return y;
}

// The facet term of a solver handle on host arrays - the Robin term of PrimalPoisson (one weight per facet, one row of
// the flux), the spring term of PrimalElasticity (three weights, two rows): `weights` and `flux` are the entries
// eqlb_*_weights and eqlb_*_flux of the handle type
template <class H, class Weights>
int32_t facet_count(H* h, Weights weights)
{
  int32_t n = 0;
  check(weights(h, &n, nullptr, 0, EQLB_MEM_HOST, nullptr));
  return n;
}
template <class H, class Weights>
darray facet_weights(H* h, int width, Weights weights)
{
  int32_t n = facet_count(h, weights);
  darray w = width == 1 ? darray((py::ssize_t)n) : darray({(py::ssize_t)n, (py::ssize_t)width});
  if (n)
    check(weights(h, &n, w.mutable_data(), n, EQLB_MEM_HOST, nullptr));
  return w;
}
// out [nlist, nq] (rows = 1) or [rows, nlist, nq]; `expected`: the message for a u_ext of another size
template <class H, class Weights, class Flux>
darray facet_flux(H* h, int rows, const darray& u, const darray& s, py::object u_ext, const char* expected,
                  Weights weights, Flux flux)
{
  const py::ssize_t n = facet_count(h, weights);
  const OptArray e = opt_array(u_ext, rows * n * s.size(), expected);
  darray out = rows == 1 ? darray({n, (py::ssize_t)s.size()}) : darray({(py::ssize_t)rows, n, (py::ssize_t)s.size()});
  check(flux(h, u.data(), (int32_t)s.size(), s.data(), e.p, out.mutable_data(), EQLB_MEM_HOST, nullptr));
  return out;
}

// -div(coeff grad u) = f on the conforming P_p space of the mesh, in the numbering of Mesh.lagrange_dofmap: operator,
// load, residual and Jacobi-preconditioned CG on the device (eqlb_primal_*), on host arrays
struct PrimalPoisson
{
  eqlb_primal_t* h = nullptr;
  std::shared_ptr<Mesh> mesh; // the handle reads the mesh: it stays alive with the carrier
  int p = 0;
  int64_t ndofs = 0;

  PrimalPoisson(std::shared_ptr<Mesh> mesh_, int p_, py::object coeff) : mesh(mesh_), p(p_)
  {
    const OptArray kc = opt_array(coeff, mesh->ncells, "PrimalPoisson: coeff [ncells] expected");
    check(eqlb_primal_create(mesh->h, p, kc.p, EQLB_MEM_HOST, nullptr, &h));
    check(eqlb_primal_ndofs(h, &ndofs));
  }
  ~PrimalPoisson() { eqlb_primal_destroy(h); }
  PrimalPoisson(const PrimalPoisson&) = delete;
  PrimalPoisson& operator=(const PrimalPoisson&) = delete;

  void need(const darray& v, const char* who) const
  {
    if (v.size() != ndofs)
      throw std::runtime_error(std::string("PrimalPoisson.") + who + ": Input sizes does not match");
  }
  void set_dirichlet(carray<int32_t> facets)
  {
    check(eqlb_primal_set_dirichlet(h, (int32_t)facets.size(), facets.size() ? facets.data() : nullptr, EQLB_MEM_HOST,
                                    nullptr));
  }
  // + c u: cell_c [ncells] where given, else the scalar c; c == 0 without an array switches the term off
  void set_reaction(double c, py::object cell_c)
  {
    const OptArray kc = opt_array(cell_c, mesh->ncells, "PrimalPoisson.set_reaction: cell_c [ncells] expected");
    check(eqlb_primal_set_reaction(h, c, kc.p, EQLB_MEM_HOST, nullptr));
  }
  // -div(coeff D grad u): cell_D [ncells][3] = (d00, d01, d11) per cell; None switches the term off
  void set_diffusion(py::object cell_D)
  {
    const OptArray kd = opt_array(cell_D, (py::ssize_t)mesh->ncells * 3,
                                  "PrimalPoisson.set_diffusion: cell_D [ncells][3] expected");
    check(eqlb_primal_set_diffusion(h, kd.p, EQLB_MEM_HOST, nullptr));
  }
  // the Robin term int alpha u v over the listed boundary facets: facet_alpha [nlist] where given, else the scalar alpha;
  // an empty list switches the term off
  void set_robin(carray<int32_t> facets, double alpha, py::object facet_alpha)
  {
    const OptArray fa = opt_array(facet_alpha, facets.size(), "PrimalPoisson.set_robin: facet_alpha [nlist] expected");
    // (an empty facet_alpha goes down as nullptr)
    check(eqlb_primal_set_robin(h, (int32_t)facets.size(), facets.size() ? facets.data() : nullptr, alpha,
                                fa.a.size() ? fa.p : nullptr, EQLB_MEM_HOST, nullptr));
  }
  darray robin_weights() const { return facet_weights(h, 1, eqlb_primal_robin_weights); }
  // out [nlist, nq] = alpha_i (u_h(x_q) - u_ext[i][q]) on the Robin list at the facet parameters s [nq]
  darray robin_flux(darray u, darray s, py::object u_ext) const
  {
    need(u, "robin_flux");
    return facet_flux(h, 1, u, s, u_ext, "PrimalPoisson.robin_flux: u_ext [nlist, nq] expected",
                      eqlb_primal_robin_weights, eqlb_primal_robin_flux);
  }
  darray load(int degree_dg, darray rhs_dg, py::object b_extra) const
  {
    if (degree_dg >= 0 && degree_dg <= 3
        && rhs_dg.size() != (py::ssize_t)mesh->ncells * ((degree_dg + 1) * (degree_dg + 2) / 2))
      throw std::runtime_error("PrimalPoisson.load: Input sizes does not match");
    const OptArray e = opt_array(b_extra, ndofs, "PrimalPoisson.load: Input sizes does not match");
    darray b((py::ssize_t)ndofs);
    check(eqlb_primal_load(h, degree_dg, rhs_dg.data(), e.p, b.mutable_data(),
                           EQLB_MEM_HOST, nullptr));
    return b;
  }
  darray apply(darray u, bool masked) const
  {
    need(u, "apply");
    darray y((py::ssize_t)ndofs);
    check(eqlb_primal_apply(h, u.data(), y.mutable_data(), masked ? 1 : 0, EQLB_MEM_HOST, nullptr));
    return y;
  }
  darray diagonal() const
  {
    darray out((py::ssize_t)ndofs);
    check(eqlb_primal_diagonal(h, out.mutable_data(), EQLB_MEM_HOST, nullptr));
    return out;
  }
  // (r, || r ||_2, nb)
  py::tuple residual(darray b, darray u) const
  {
    need(b, "residual");
    need(u, "residual");
    darray r((py::ssize_t)ndofs);
    double norms[2] = {0.0, 0.0};
    check(eqlb_primal_residual(h, b.data(), u.data(), r.mutable_data(), norms, EQLB_MEM_HOST, nullptr));
    return py::make_tuple(r, norms[0], norms[1]);
  }
  // (u, info): the solution from the start u (its fixed rows hold the Dirichlet values) and the info dict
  py::tuple solve(darray b, darray u, double rtol, double atol, int maxit) const
  {
    need(b, "solve");
    need(u, "solve");
    darray x((py::ssize_t)ndofs);
    std::copy(u.data(), u.data() + ndofs, x.mutable_data());
    double v[8] = {};
    check(eqlb_primal_solve(h, b.data(), x.mutable_data(), rtol, atol, maxit, v, EQLB_MEM_HOST, nullptr));
    py::dict info;
    info["iterations"] = (int64_t)v[0];
    info["converged"] = (int64_t)v[1];
    info["nb"] = v[2];
    info["rnorm"] = v[3];
    info["replacements"] = (int64_t)v[4];
    info["breakdown"] = (int64_t)v[5];
    info["tol"] = v[6];
    info["facets_skipped"] = (int64_t)v[7];
    return py::make_tuple(x, info);
  }
  // the operator as CSR: (indptr, indices, values); the pattern is built at the first call and kept in the handle
  py::tuple matrix(bool eliminate) const
  {
    return matrix_of(h, ndofs, eliminate, eqlb_primal_matrix_pattern, eqlb_primal_matrix_export,
                     eqlb_primal_matrix_values);
  }
  darray matrix_values(bool eliminate) const
  {
    return matrix_values_of(h, eliminate, eqlb_primal_matrix_pattern, eqlb_primal_matrix_values);
  }
  void matrix_release() { eqlb_primal_matrix_release(h); }
  // Y [nrhs][ndofs]: row c is apply(U[c])
  darray apply_many(darray U, bool masked) const
  {
    const int32_t nrhs = many_columns(U, ndofs, "PrimalPoisson.apply_many");
    darray y({(py::ssize_t)nrhs, (py::ssize_t)ndofs});
    check(eqlb_primal_apply_many(h, nrhs, U.data(), y.mutable_data(), masked ? 1 : 0, EQLB_MEM_HOST, nullptr));
    return y;
  }
  // (U, infos): row c and infos[c] are solve(B[c], U[c])
  py::tuple solve_many(darray B, darray U, double rtol, double atol, int maxit) const
  {
    const int32_t nrhs = many_columns(B, ndofs, "PrimalPoisson.solve_many");
    if (many_columns(U, ndofs, "PrimalPoisson.solve_many") != nrhs)
      throw std::runtime_error("PrimalPoisson.solve_many: Input sizes does not match");
    darray x({(py::ssize_t)nrhs, (py::ssize_t)ndofs});
    std::copy(U.data(), U.data() + (int64_t)nrhs * ndofs, x.mutable_data());
    std::vector<double> v(8 * (size_t)nrhs, 0.0);
    check(eqlb_primal_solve_many(h, nrhs, B.data(), x.mutable_data(), rtol, atol, maxit, v.data(), EQLB_MEM_HOST,
                                 nullptr));
    return py::make_tuple(x, many_info(v));
  }
};

// -div(2 eps(u) + pi_1 div(u) I) = f on [P_p]^2 in the scalar numbering of Mesh.lagrange_dofmap, blocked x[2 dof + r]:
// the counterpart of PrimalPoisson (eqlb_elasticity_*), on host arrays; ndofs is the scalar count, vectors have 2 ndofs
struct PrimalElasticity
{
  eqlb_elasticity_t* h = nullptr;
  std::shared_ptr<Mesh> mesh; // the handle reads the mesh: it stays alive with the carrier
  int p = 0;
  int64_t ndofs = 0;

  PrimalElasticity(std::shared_ptr<Mesh> mesh_, int p_, double pi_1, py::object cell_pi1) : mesh(mesh_), p(p_)
  {
    const OptArray kc = opt_array(cell_pi1, mesh->ncells, "PrimalElasticity: cell_pi1 [ncells] expected");
    check(eqlb_elasticity_create(mesh->h, p, pi_1, kc.p, EQLB_MEM_HOST, nullptr, &h));
    check(eqlb_elasticity_ndofs(h, &ndofs));
  }
  ~PrimalElasticity() { eqlb_elasticity_destroy(h); }
  PrimalElasticity(const PrimalElasticity&) = delete;
  PrimalElasticity& operator=(const PrimalElasticity&) = delete;

  void need(const darray& v, const char* who) const
  {
    if (v.size() != 2 * ndofs)
      throw std::runtime_error(std::string("PrimalElasticity.") + who + ": Input sizes does not match");
  }
  void set_dirichlet(carray<int32_t> facets0, carray<int32_t> facets1)
  {
    check(eqlb_elasticity_set_dirichlet(h, (int32_t)facets0.size(), facets0.size() ? facets0.data() : nullptr,
                                        (int32_t)facets1.size(), facets1.size() ? facets1.data() : nullptr,
                                        EQLB_MEM_HOST, nullptr));
  }
  // + c u: cell_c [ncells] where given, else the scalar c; c == 0 without an array switches the term off
  void set_reaction(double c, py::object cell_c)
  {
    const OptArray kc = opt_array(cell_c, mesh->ncells, "PrimalElasticity.set_reaction: cell_c [ncells] expected");
    check(eqlb_elasticity_set_reaction(h, c, kc.p, EQLB_MEM_HOST, nullptr));
  }
  // sigma = mu (2 eps(u) + pi_1 div(u) I): cell_mu [ncells] where given, else the scalar mu; mu == 1 without an array
  // switches the term off
  void set_shear(double mu, py::object cell_mu)
  {
    const OptArray kc = opt_array(cell_mu, mesh->ncells, "PrimalElasticity.set_shear: cell_mu [ncells] expected");
    check(eqlb_elasticity_set_shear(h, mu, kc.p, EQLB_MEM_HOST, nullptr));
  }
  // the spring term int_E v^T K u over the listed boundary facets: facet_k [nlist, 3] = (k00, k01, k11) where given,
  // else k I; an empty list switches the term off
  void set_springs(carray<int32_t> facets, double k, py::object facet_k)
  {
    carray<double> fk;
    if (!facet_k.is_none())
    {
      fk = facet_k.cast<carray<double>>();
      if (fk.size() != 3 * facets.size())
        throw std::runtime_error("PrimalElasticity.set_springs: facet_k [nlist, 3] expected");
    }
    check(eqlb_elasticity_set_springs(h, (int32_t)facets.size(), facets.size() ? facets.data() : nullptr, k,
                                      !facet_k.is_none() && fk.size() ? fk.data() : nullptr, EQLB_MEM_HOST, nullptr));
  }
  int spring_count() const { return facet_count(h, eqlb_elasticity_spring_weights); }
  darray spring_weights() const { return facet_weights(h, 3, eqlb_elasticity_spring_weights); }
  // out [2, nlist, nq] = K_i (u_h(x_q) - u_ext[.][i][q]) on the spring list at the facet parameters s [nq]
  darray spring_flux(darray u, darray s, py::object u_ext) const
  {
    need(u, "spring_flux");
    return facet_flux(h, 2, u, s, u_ext, "PrimalElasticity.spring_flux: u_ext [2, nlist, nq] expected",
                      eqlb_elasticity_spring_weights, eqlb_elasticity_spring_flux);
  }
  darray load(int degree_dg, darray rhs_dg, py::object b_extra) const
  {
    if (degree_dg >= 0 && degree_dg <= 3
        && rhs_dg.size() != 2 * (py::ssize_t)mesh->ncells * ((degree_dg + 1) * (degree_dg + 2) / 2))
      throw std::runtime_error("PrimalElasticity.load: Input sizes does not match");
    const OptArray e = opt_array(b_extra, 2 * ndofs, "PrimalElasticity.load: Input sizes does not match");
    darray b((py::ssize_t)(2 * ndofs));
    check(eqlb_elasticity_load(h, degree_dg, rhs_dg.data(), e.p, b.mutable_data(),
                               EQLB_MEM_HOST, nullptr));
    return b;
  }
  darray apply(darray u, bool masked) const
  {
    need(u, "apply");
    darray y((py::ssize_t)(2 * ndofs));
    check(eqlb_elasticity_apply(h, u.data(), y.mutable_data(), masked ? 1 : 0, EQLB_MEM_HOST, nullptr));
    return y;
  }
  darray diagonal() const
  {
    darray out((py::ssize_t)(2 * ndofs));
    check(eqlb_elasticity_diagonal(h, out.mutable_data(), EQLB_MEM_HOST, nullptr));
    return out;
  }
  // (r, || r ||_2, nb)
  py::tuple residual(darray b, darray u) const
  {
    need(b, "residual");
    need(u, "residual");
    darray r((py::ssize_t)(2 * ndofs));
    double norms[2] = {0.0, 0.0};
    check(eqlb_elasticity_residual(h, b.data(), u.data(), r.mutable_data(), norms, EQLB_MEM_HOST, nullptr));
    return py::make_tuple(r, norms[0], norms[1]);
  }
  // the operator as CSR: (indptr, indices, values), 2 ndofs rows; the pattern is built at the first call and kept
  py::tuple matrix(bool eliminate) const
  {
    return matrix_of(h, 2 * ndofs, eliminate, eqlb_elasticity_matrix_pattern, eqlb_elasticity_matrix_export,
                     eqlb_elasticity_matrix_values);
  }
  darray matrix_values(bool eliminate) const
  {
    return matrix_values_of(h, eliminate, eqlb_elasticity_matrix_pattern, eqlb_elasticity_matrix_values);
  }
  void matrix_release() { eqlb_elasticity_matrix_release(h); }
  // (u, info): the solution from the start u (its fixed rows hold the Dirichlet values) and the info dict
  py::tuple solve(darray b, darray u, double rtol, double atol, int maxit) const
  {
    need(b, "solve");
    need(u, "solve");
    darray x((py::ssize_t)(2 * ndofs));
    std::copy(u.data(), u.data() + 2 * ndofs, x.mutable_data());
    double v[8] = {};
    check(eqlb_elasticity_solve(h, b.data(), x.mutable_data(), rtol, atol, maxit, v, EQLB_MEM_HOST, nullptr));
    py::dict info;
    info["iterations"] = (int64_t)v[0];
    info["converged"] = (int64_t)v[1];
    info["nb"] = v[2];
    info["rnorm"] = v[3];
    info["replacements"] = (int64_t)v[4];
    info["breakdown"] = (int64_t)v[5];
    info["tol"] = v[6];
    info["facets_skipped"] = (int64_t)v[7];
    return py::make_tuple(x, info);
  }
};

// The multilevel preconditioner over the levels of an adaptive loop (eqlb_hierarchy_*), on host arrays: solvers coarsest
// first, all PrimalPoisson or all PrimalElasticity; transfers[l] the Transfer of Mesh.refine(..., keep_plan=True) from
// the mesh of solvers[l] to that of solvers[l + 1]
struct Multilevel
{
  eqlb_hierarchy_t* h = nullptr;
  py::list keep_solvers, keep_transfers; // everything is borrowed: it stays alive with the carrier
  int bs = 1, nlevels = 0;
  bool local = false;                    // local smoothing (eqlb_hierarchy_set_local)
  bool coarse = false;                   // exact solve on level 0 (eqlb_hierarchy_set_coarse)
  std::vector<int64_t> n;                // rows of a vector per level

  Multilevel(py::list solvers, py::list transfers, bool local_, bool coarse_)
      : keep_solvers(solvers), keep_transfers(transfers)
  {
    nlevels = (int)py::len(solvers);
    if (nlevels < 1 || (int)py::len(transfers) != nlevels - 1)
      throw std::runtime_error("Multilevel: one Transfer per pair of neighbouring levels expected");
    const bool el = py::isinstance<PrimalElasticity>(solvers[0]);
    bs = el ? 2 : 1;
    std::vector<void*> sv;
    std::vector<eqlb_mesh_t*> ms;
    std::vector<eqlb_refine_t*> pl;
    for (int l = 0; l < nlevels; ++l)
    {
      if (el)
      {
        auto s = solvers[l].cast<std::shared_ptr<PrimalElasticity>>();
        sv.push_back(s->h), ms.push_back(s->mesh->h), n.push_back(2 * s->ndofs);
      }
      else
      {
        auto s = solvers[l].cast<std::shared_ptr<PrimalPoisson>>();
        sv.push_back(s->h), ms.push_back(s->mesh->h), n.push_back(s->ndofs);
      }
      if (l < nlevels - 1)
        pl.push_back(transfers[l].cast<std::shared_ptr<Transfer>>()->plan);
    }
    check(eqlb_hierarchy_create(nlevels, bs, sv.data(), pl.data(), ms.data(), nullptr, &h));
    if (local_)
    {
      const int st = eqlb_hierarchy_set_local(h, 1, nullptr);
      if (st != EQLB_OK)
        eqlb_hierarchy_destroy(h); // (the destructor of an object whose constructor throws does not run)
      check(st);
      local = true;
    }
    if (coarse_)
    {
      const int st = eqlb_hierarchy_set_coarse(h, 1, nullptr);
      if (st != EQLB_OK)
        eqlb_hierarchy_destroy(h);
      check(st);
      coarse = true;
    }
  }
  ~Multilevel() { eqlb_hierarchy_destroy(h); }
  Multilevel(const Multilevel&) = delete;
  Multilevel& operator=(const Multilevel&) = delete;

  void set_local(bool on)
  {
    check(eqlb_hierarchy_set_local(h, on ? 1 : 0, nullptr));
    local = on;
  }
  // (switching on factors level 0, again if it was on; a refusal leaves the switch off)
  void set_coarse(bool on)
  {
    if (on)
      coarse = false;
    check(eqlb_hierarchy_set_coarse(h, on ? 1 : 0, nullptr));
    coarse = on;
  }
  int64_t coarse_rows() const
  {
    int64_t c = 0;
    check(eqlb_hierarchy_coarse_rows(h, &c));
    return c;
  }
  // (rows, d, W) of the factor of level 0
  py::tuple coarse_factor() const
  {
    const int64_t c = coarse_rows();
    py::array_t<int32_t> rows((py::ssize_t)c);
    darray d((py::ssize_t)c);
    py::array_t<double, py::array::c_style> W({(py::ssize_t)c, (py::ssize_t)c});
    check(eqlb_hierarchy_coarse_factor(h, rows.mutable_data(), d.mutable_data(), W.mutable_data(), c, EQLB_MEM_HOST,
                                       nullptr));
    return py::make_tuple(rows, d, W);
  }
  // the rows the local rule smooths on `level`
  py::array_t<bool> active(int level) const
  {
    const bool ok = level >= 0 && level < nlevels;
    std::vector<uint8_t> v((size_t)(ok ? n[level] : 1));
    check(eqlb_hierarchy_active(h, level, v.data(), (int64_t)v.size(), EQLB_MEM_HOST, nullptr));
    py::array_t<bool> out((py::ssize_t)v.size());
    bool* o = out.mutable_data();
    for (size_t i = 0; i < v.size(); ++i)
      o[i] = v[i] != 0;
    return out;
  }
  int64_t active_count(int level) const
  {
    int64_t c = 0;
    check(eqlb_hierarchy_active_count(h, level, &c));
    return c;
  }
  // level + 1 -> level
  darray restrict(int level, darray r, bool masked) const
  {
    if (level >= 0 && level < nlevels - 1 && r.size() != n[level + 1])
      throw std::runtime_error("Multilevel.restrict: Input sizes does not match");
    darray out((py::ssize_t)(level >= 0 && level < nlevels - 1 ? n[level] : 1));
    check(eqlb_hierarchy_restrict(h, level, r.data(), out.mutable_data(), masked ? 1 : 0, EQLB_MEM_HOST, nullptr));
    return out;
  }
  darray precondition(darray r) const
  {
    if (r.size() != n.back())
      throw std::runtime_error("Multilevel.precondition: Input sizes does not match");
    darray z((py::ssize_t)n.back());
    check(eqlb_hierarchy_precondition(h, r.data(), z.mutable_data(), EQLB_MEM_HOST, nullptr));
    return z;
  }
  py::tuple solve(darray b, darray u, double rtol, double atol, int maxit) const
  {
    if (b.size() != n.back() || u.size() != n.back())
      throw std::runtime_error("Multilevel.solve: Input sizes does not match");
    darray x((py::ssize_t)n.back());
    std::copy(u.data(), u.data() + n.back(), x.mutable_data());
    double v[8] = {};
    check(eqlb_hierarchy_solve(h, b.data(), x.mutable_data(), rtol, atol, maxit, v, EQLB_MEM_HOST, nullptr));
    py::dict info;
    info["iterations"] = (int64_t)v[0];
    info["converged"] = (int64_t)v[1];
    info["nb"] = v[2];
    info["rnorm"] = v[3];
    info["replacements"] = (int64_t)v[4];
    info["breakdown"] = (int64_t)v[5];
    info["tol"] = v[6];
    info["facets_skipped"] = (int64_t)v[7];
    return py::make_tuple(x, info);
  }
  // Z [nrhs][n]: row c is precondition(R[c]) (Poisson handles only)
  darray precondition_many(darray R) const
  {
    const int32_t nrhs = many_columns(R, n.back(), "Multilevel.precondition_many");
    darray z({(py::ssize_t)nrhs, (py::ssize_t)n.back()});
    check(eqlb_hierarchy_precondition_many(h, nrhs, R.data(), z.mutable_data(), EQLB_MEM_HOST, nullptr));
    return z;
  }
  // (U, infos): row c and infos[c] are solve(B[c], U[c]) (Poisson handles only)
  py::tuple solve_many(darray B, darray U, double rtol, double atol, int maxit) const
  {
    const int32_t nrhs = many_columns(B, n.back(), "Multilevel.solve_many");
    if (many_columns(U, n.back(), "Multilevel.solve_many") != nrhs)
      throw std::runtime_error("Multilevel.solve_many: Input sizes does not match");
    darray x({(py::ssize_t)nrhs, (py::ssize_t)n.back()});
    std::copy(U.data(), U.data() + (int64_t)nrhs * n.back(), x.mutable_data());
    std::vector<double> v(8 * (size_t)nrhs, 0.0);
    check(eqlb_hierarchy_solve_many(h, nrhs, B.data(), x.mutable_data(), rtol, atol, maxit, v.data(), EQLB_MEM_HOST,
                                    nullptr));
    return py::make_tuple(x, many_info(v));
  }
};

py::tuple Mesh::refine(std::shared_ptr<Mesh> self, carray<int32_t> marked, bool keep_plan)
{
  std::shared_ptr<Transfer> tr(new Transfer());
  tr->coarse = self;
  const int64_t nmarked = (int64_t)marked.size();
  check(eqlb_mesh_refine_plan(self->h, marked.data(), &nmarked, nmarked, EQLB_MEM_HOST, nullptr, &tr->plan));
  std::shared_ptr<Mesh> m(new Mesh());
  int32_t nbis = 0;
  check(eqlb_refine_counts(tr->plan, &m->nnodes, &m->ncells, &nbis, nullptr));
  m->x.resize(3 * (size_t)m->nnodes);
  m->cell_nodes.resize(3 * (size_t)m->ncells);
  py::array_t<int32_t> parent_cell(m->ncells), node_parent_facet(nbis);
  check(eqlb_refine_write(tr->plan, m->x.data(), m->cell_nodes.data(), parent_cell.mutable_data(),
                          node_parent_facet.mutable_data(), EQLB_MEM_HOST, nullptr));
  check(eqlb_refine_create_mesh(tr->plan, nullptr, &m->h));
  m->export_tables();
  py::array_t<int32_t> parent_facet(m->nfacets);
  check(eqlb_refine_parent_facets(tr->plan, m->h, parent_facet.mutable_data(), EQLB_MEM_HOST, nullptr));
  if (!keep_plan)
    return py::make_tuple(m, parent_cell, node_parent_facet, parent_facet);
  tr->fine = m;
  return py::make_tuple(m, parent_cell, node_parent_facet, parent_facet, tr);
}

// family "DG": discontinuous Lagrange P_degree (block size bs); family "RT": the hierarchic RT_degree of
// create_hierarchic_rt (elmtlib/e_raviart_thomas.py:14-196) - discontinuous: global DOF = cell * k(k+2) +
// local (the semi-explicit flux space, FluxEqlbSE.py:98-101); conforming: k DOFs per facet in the global
// facet frame, then k^2 - k per cell (stand-in of the Basix RT_k space of FluxEqlbEV.py:100), numbered
// facet * k + j, nfacets * k + cell * (k^2 - k) + i unless a cell -> DOF table is given
struct FunctionSpace
{
  std::shared_ptr<Mesh> mesh;
  std::string family;
  int degree, bs;
  bool discontinuous;
  std::vector<int32_t> cell_dofs; // conforming RT only, optional
  int64_t ndofs_user = 0;

  FunctionSpace(std::shared_ptr<Mesh> m, std::string fam, int deg, int bs_, bool disc)
      : mesh(std::move(m)), family(std::move(fam)), degree(deg), bs(bs_), discontinuous(disc)
  {
    if (!mesh)
      throw std::runtime_error("FunctionSpace: mesh is None");
    if (family != "DG" && family != "RT")
      throw std::runtime_error("FunctionSpace: family must be 'DG' or 'RT'");
    if (family == "DG" && (degree < 0 || !discontinuous))
      throw std::runtime_error("FunctionSpace: DG spaces are discontinuous, degree >= 0");
    if (family == "RT" && (degree < 1 || bs != 1))
      throw std::runtime_error("FunctionSpace: RT_k needs k >= 1 and block size 1");
  }
  int ndofs_cell() const
  {
    return family == "DG" ? (degree + 1) * (degree + 2) / 2 : degree * (degree + 2);
  }
  int64_t ndofs() const // scalar DOFs x block size
  {
    if (family == "DG" || discontinuous)
      return (int64_t)mesh->ncells * ndofs_cell() * bs;
    if (!cell_dofs.empty())
      return ndofs_user;
    return (int64_t)mesh->nfacets * degree + (int64_t)mesh->ncells * (degree * degree - degree);
  }
  void set_dofmap(carray<int32_t> cd, int64_t n)
  {
    if (family != "RT" || discontinuous)
      throw std::runtime_error("FunctionSpace.set_dofmap: conforming RT spaces only");
    if (cd.size() != (py::ssize_t)mesh->ncells * ndofs_cell())
      throw std::runtime_error("FunctionSpace.set_dofmap: cell_dofs [ncells, k(k+2)] expected");
    cell_dofs.assign(cd.data(), cd.data() + cd.size());
    ndofs_user = n;
  }
};

struct Function
{
  std::shared_ptr<FunctionSpace> V;
  py::array_t<double> host; // owned or caller's array (zero copy)
  uintptr_t dev = 0;        // device pointer (from_device)
  bool on_device = false;

  explicit Function(std::shared_ptr<FunctionSpace> V_) : V(std::move(V_))
  {
    if (!V)
      throw std::runtime_error("Function: function space is None");
    host = py::array_t<double>(V->ndofs());
    std::fill_n(host.mutable_data(), host.size(), 0.0);
  }
  Function(std::shared_ptr<FunctionSpace> V_, py::array_t<double> a) : V(std::move(V_)), host(std::move(a))
  {
    if (!V)
      throw std::runtime_error("Function: function space is None");
    if (!(host.flags() & py::array::c_style) || !host.writeable() || host.size() != V->ndofs())
      throw std::runtime_error("Function: a writeable C-contiguous float64 array of the size of the space is required");
  }
  static std::shared_ptr<Function> from_device(std::shared_ptr<FunctionSpace> V, uintptr_t ptr)
  {
    if (!ptr)
      throw std::runtime_error("Function.from_device: null pointer");
    auto f = std::shared_ptr<Function>(new Function());
    f->V = std::move(V);
    f->dev = ptr;
    f->on_device = true;
    return f;
  }
  double* data() { return on_device ? reinterpret_cast<double*>(dev) : host.mutable_data(); }
  int64_t size() const { return V->ndofs(); }

private:
  Function() = default;
};

struct Constant
{
  std::vector<double> value;
  explicit Constant(carray<double> v) : value(v.data(), v.data() + v.size()) {}
};

// A compiled form of the reference is fixed by the call it is handed to (FluxEqlbEV.py:113-134: a, l_pen,
// l_i; lsolver/projection.py:54-66: a = (u, v), l_i = (f_i, v)); what varies is its data:
//   Form(coefficients)                       the Functions the form depends on (l_i of EV: [G_i, f_i])
//   Form.from_point_values(qp, qw, values)   l_i of the projector: f_i at the images of a reference rule
struct Form
{
  std::vector<std::shared_ptr<Function>> coefficients;
  darray qpoints, qweights, qvalues;
  bool has_points = false;
  explicit Form(std::vector<std::shared_ptr<Function>> c) : coefficients(std::move(c)) {}
  static std::shared_ptr<Form> from_point_values(darray qp, darray qw, darray qv)
  {
    auto f = std::make_shared<Form>(std::vector<std::shared_ptr<Function>>{});
    if (qp.ndim() != 2 || qp.shape(1) != 2 || qw.size() != qp.shape(0))
      throw std::runtime_error("Form.from_point_values: qpoints [nq, 2], qweights [nq] expected");
    f->qpoints = std::move(qp);
    f->qweights = std::move(qw);
    f->qvalues = std::move(qv);
    f->has_points = true;
    return f;
  }
};

// Gauss-Legendre rule on [0, 1] exact for `degree` (basix.make_quadrature(interval, degree): m = (degree+2)/2)
void facet_rule(int degree, std::vector<double>& s, std::vector<double>& w)
{
  const int m = std::max(1, (degree + 2) / 2);
  s.resize(m);
  w.resize(m);
  const double pi = 3.14159265358979323846;
  for (int i = 0; i < m; ++i)
  {
    double z = std::cos(pi * (i + 0.75) / (m + 0.5)), pp = 1.0;
    for (int it = 0; it < 100; ++it)
    {
      double p1 = 1.0, p2 = 0.0;
      for (int j = 1; j <= m; ++j)
      {
        const double p3 = p2;
        p2 = p1;
        p1 = ((2.0 * j - 1.0) * z * p2 - (j - 1.0) * p3) / j;
      }
      pp = m * (z * p1 - p2) / (z * z - 1.0);
      const double dz = p1 / pp;
      z -= dz;
      if (std::fabs(dz) < 1e-15)
        break;
    }
    s[m - 1 - i] = 0.5 * (1.0 + z);
    w[m - 1 - i] = 1.0 / ((1.0 - z * z) * pp * pp);
  }
}

// interpolation rule of the hierarchic RT_k facet functionals (e_raviart_thomas.py:63-71)
inline int interpolation_degree(int k) { return k == 1 ? 1 : 2 * k; }

using bkernel_t = void (*)(double*, const double*, const double*, const double*, const int*, const uint8_t*);

struct FluxBC
{
  std::shared_ptr<FunctionSpace> V;
  std::vector<int32_t> facets;
  bkernel_t kernel;
  int nevals, qdegree;
  bool projection;
  std::vector<std::shared_ptr<Function>> coefficients;
  std::vector<int> positions;
  std::vector<std::shared_ptr<Constant>> constants;

  FluxBC(std::shared_ptr<FunctionSpace> V_, std::vector<int32_t> fcts, uintptr_t kptr, int nev, int qdeg,
         bool proj, std::vector<std::shared_ptr<Function>> coeffs, std::vector<int> pos,
         std::vector<std::shared_ptr<Constant>> consts)
      : V(std::move(V_)), facets(std::move(fcts)), kernel(reinterpret_cast<bkernel_t>(kptr)), nevals(nev),
        qdegree(qdeg), projection(proj), coefficients(std::move(coeffs)), positions(std::move(pos)),
        constants(std::move(consts))
  {
    if (!V)
      throw std::runtime_error("FluxBC: function space is None");
    for (const auto& c : coefficients)
      if (!c || c->on_device || c->V->family != "DG")
        throw std::runtime_error("FluxBC: coefficients are host Functions of DG spaces");
  }
};

inline double binom(int n, int r)
{
  double v = 1.0;
  for (int i = 0; i < r; ++i)
    v = v * (n - i) / (i + 1);
  return v;
}
// T_f of the conforming hierarchic RT_k: -I (facet_perm 0) or B_ji = C(j,i)(-1)^i; an involution
inline double facet_map(bool rev, int j, int i)
{
  if (!rev)
    return (i == j) ? -1.0 : 0.0;
  return (i > j) ? 0.0 : ((i % 2 == 0) ? 1.0 : -1.0) * binom(j, i);
}

struct BoundaryData
{
  std::shared_ptr<FunctionSpace> V;
  std::shared_ptr<Mesh> mesh;
  int k, nrhs;
  bool custom, stress;
  std::vector<int8_t> facet_type;      // [nrhs][nfacets]
  std::vector<double> boundary_values; // [nrhs][ndofs], empty: homogeneous
  std::vector<std::shared_ptr<Function>> boundary_flux;
  std::vector<std::vector<std::shared_ptr<FluxBC>>> bcs; // the conditions, kept for update()
  int qdegree;                                           // rule of the projected conditions
  // device handles, created with the first equilibration call (the degree of the projected data is
  // known only then, se/reconstruction.hpp:363-373) and kept
  eqlb_se_t* se = nullptr;
  eqlb_ev_t* ev = nullptr;
  std::vector<double> basis_C, basis_R;
  int se_degree_dg = -1;
  int ev_degree_dg = -1;
  // options set through set_option: applied behind eqlb_*_create and before eqlb_*_set_boundary, so they also reach
  // a handle that does not exist yet or is rebuilt for another degree ("large_patches" and "large_patches_stress" act
  // in set_boundary)
  std::vector<std::pair<std::string, int>> se_options, ev_options;

  BoundaryData(std::vector<std::vector<std::shared_ptr<FluxBC>>>& list_bcs,
               std::vector<std::shared_ptr<Function>>& bflux, std::shared_ptr<FunctionSpace> V_, bool rt_custom,
               int quadrature_degree, const std::vector<std::vector<int32_t>>& fct_esntbound_prime, bool rstress)
      : V(std::move(V_)), custom(rt_custom), stress(rstress), boundary_flux(bflux), bcs(list_bcs),
        qdegree(quadrature_degree)
  {
    if (!V || V->family != "RT")
      throw std::runtime_error("BoundaryData: V_flux_hdiv must be an RT space");
    if (custom != V->discontinuous)
      throw std::runtime_error("BoundaryData: rtflux_is_custom must match the flux space (discontinuous "
                               "hierarchic RT_k for the semi-explicit equilibrator)");
    mesh = V->mesh;
    k = V->degree;
    nrhs = (int)list_bcs.size();
    if ((int)bflux.size() != nrhs || (int)fct_esntbound_prime.size() != nrhs)
      throw std::runtime_error("Size of input data does not match!");
    const int64_t ndofs = V->ndofs();
    facet_type.assign((size_t)nrhs * mesh->nfacets, (int8_t)EQLB_FACET_INTERNAL);
    for (int r = 0; r < nrhs; ++r)
    {
      if (!bflux[r] || bflux[r]->on_device || bflux[r]->size() != ndofs)
        throw std::runtime_error("BoundaryData: boundary functions are host Functions of V_flux_hdiv");
      int8_t* ft = &facet_type[(size_t)r * mesh->nfacets];
      for (int32_t f : fct_esntbound_prime[r])
      {
        if (f < 0 || f >= mesh->nfacets)
          throw std::runtime_error("BoundaryData: facet index out of range");
        ft[f] = EQLB_FACET_ESSNT_PRIMAL;
      }
    }
    if (evaluate(nullptr, nullptr))
      store_boundary_values();
  }
  void store_boundary_values()
  {
    const int64_t ndofs = V->ndofs();
    boundary_values.resize((size_t)nrhs * ndofs);
    for (int r = 0; r < nrhs; ++r)
      std::copy_n(boundary_flux[r]->data(), ndofs, &boundary_values[(size_t)r * ndofs]);
  }
  // The FluxBC kernels with their current constants and coefficients -> facet types and boundary functions.  Returns
  // whether any DOF is non-zero.  facets / moments (per right-hand side, or nullptr): the flux-BC facets that carry a
  // kernel and their k DOFs in the frame of the facet's cell, as eqlb_*_update_flux_bc takes them.
  bool evaluate(std::vector<std::vector<int32_t>>* facets, std::vector<std::vector<double>>* moments)
  {
    const int nrt = k * (k + 2);
    bool inhomogeneous = false;
    std::vector<double> sq, wq, vals, cdata, coefs;
    for (int r = 0; r < nrhs; ++r)
    {
      int8_t* ft = &facet_type[(size_t)r * mesh->nfacets];
      double* xb = boundary_flux[r]->data();
      for (const auto& bc : bcs[r])
      {
        // base/BoundaryData.cpp:437-445: the number of evaluation points must fit the rule in use
        facet_rule(bc->projection ? qdegree : interpolation_degree(k), sq, wq);
        const int nq = (int)sq.size();
        if (nq != bc->nevals)
          throw std::runtime_error("BoundaryData: Number of evaluation points (FluxBC) does not match!");
        cdata.clear();
        for (const auto& c : bc->constants)
          cdata.insert(cdata.end(), c->value.begin(), c->value.end());
        vals.assign((size_t)3 * nq, 0.0);
        for (int32_t fct : bc->facets)
        {
          if (fct < 0 || fct >= mesh->nfacets
              || mesh->facet_cells_off[fct + 1] - mesh->facet_cells_off[fct] != 1)
            throw std::runtime_error("BoundaryData: flux BCs live on boundary facets");
          const int32_t cell = mesh->facet_cells[mesh->facet_cells_off[fct]];
          int lf = 0;
          for (int l = 1; l < 3; ++l)
            if (mesh->cell_facets[3 * (size_t)cell + l] == fct)
              lf = l;
          ft[fct] = EQLB_FACET_ESSNT_DUAL;
          if (!bc->kernel)
            continue; // homogeneous condition (no kernel: zero flux)
          double coords[9];
          for (int v = 0; v < 3; ++v)
            for (int d = 0; d < 3; ++d)
              coords[3 * v + d] = mesh->x[3 * (size_t)mesh->cell_nodes[3 * (size_t)cell + v] + d];
          coefs.clear(); // cell DOFs of the coefficients (FluxBC::extract_coefficients)
          for (const auto& c : bc->coefficients)
          {
            const int n = c->V->ndofs_cell() * c->V->bs;
            const double* p = c->data() + (size_t)cell * n;
            coefs.insert(coefs.end(), p, p + n);
          }
          std::fill(vals.begin(), vals.end(), 0.0);
          bc->kernel(vals.data(), coefs.data(), cdata.data(), coords, nullptr, nullptr);
          // DOF_j = pf_f sign(detJ) |E| int_0^1 g s^j ds : the functional int (detJ K w) . N_f s^j ds of
          // the element for a field with w . n = g (L2 projection of the normal trace and interpolation
          // coincide on the moments, base/BoundaryData.cpp:470-575)
          double J[2][2];
          const double detJ = mesh->jacobian(cell, J);
          const int32_t va = mesh->cell_nodes[3 * (size_t)cell + (lf == 0 ? 1 : 0)];
          const int32_t vb = mesh->cell_nodes[3 * (size_t)cell + (lf == 2 ? 1 : 2)];
          const double ex = mesh->x[3 * (size_t)vb] - mesh->x[3 * (size_t)va];
          const double ey = mesh->x[3 * (size_t)vb + 1] - mesh->x[3 * (size_t)va + 1];
          const double scale = ((lf == 1) ? 1.0 : -1.0) * ((detJ > 0.0) ? 1.0 : -1.0) * std::sqrt(ex * ex + ey * ey);
          double dof[16];
          for (int j = 0; j < k; ++j)
          {
            double acc = 0.0;
            for (int q = 0; q < nq; ++q)
              acc += wq[q] * vals[(size_t)lf * nq + q] * std::pow(sq[q], j);
            dof[j] = scale * acc;
            inhomogeneous = inhomogeneous || dof[j] != 0.0;
          }
          if (facets)
          {
            (*facets)[r].push_back(fct);
            (*moments)[r].insert((*moments)[r].end(), dof, dof + k);
          }
          if (custom)
            for (int j = 0; j < k; ++j)
              xb[(size_t)cell * nrt + lf * k + j] = dof[j];
          else
          {
            const bool rev = mesh->facet_perm[3 * (size_t)cell + lf] != 0;
            for (int j = 0; j < k; ++j)
            {
              double g = 0.0;
              for (int i = 0; i < k; ++i)
                g += facet_map(rev, j, i) * dof[i];
              const int64_t d = V->cell_dofs.empty() ? (int64_t)fct * k + j
                                                     : (int64_t)V->cell_dofs[(size_t)cell * nrt + lf * k + j];
              xb[d] = g;
            }
          }
        }
      }
    }
    return inhomogeneous;
  }
  // New values of the flux BCs on unchanged facets (a load step, a time step): the kernels are evaluated again, and
  // a device handle that exists receives the facet DOFs through eqlb_*_update_flux_bc - its patches, bins and tiles
  // stay.  A handle created later reads boundary_values as before.
  void update()
  {
    std::vector<std::vector<int32_t>> fl(nrhs);
    std::vector<std::vector<double>> fd(nrhs);
    if (evaluate(&fl, &fd) || !boundary_values.empty())
      store_boundary_values();
    try
    {
      for (int r = 0; r < nrhs; ++r)
      {
        const int32_t n = (int32_t)fl[r].size();
        if (n == 0)
          continue;
        if (se)
          check(eqlb_se_update_flux_bc(se, r, n, fl[r].data(), 0, nullptr, nullptr, fd[r].data(), 0, nullptr,
                                       EQLB_MEM_HOST, g_stream));
        if (ev)
          check(eqlb_ev_update_flux_bc(ev, r, n, fl[r].data(), 0, nullptr, nullptr, fd[r].data(), 0, nullptr,
                                       EQLB_MEM_HOST, g_stream));
      }
    }
    catch (...)
    {
      // no handle with a half-written table is kept: the next call rebuilds it from boundary_values
      eqlb_se_destroy(se);
      eqlb_ev_destroy(ev);
      se = nullptr;
      ev = nullptr;
      throw;
    }
  }
  ~BoundaryData()
  {
    eqlb_se_destroy(se);
    eqlb_ev_destroy(ev);
  }
  BoundaryData(const BoundaryData&) = delete;
  BoundaryData& operator=(const BoundaryData&) = delete;

  eqlb_se_t* se_handle(int degree_dg, bool rstress)
  {
    if (!custom)
      throw std::runtime_error("reconstruct_fluxes_semiexplt: the boundary data belongs to a conforming flux space");
    if (rstress != stress)
      throw std::runtime_error("reconstruct_stress does not match the BoundaryData");
    if (se && se_degree_dg == degree_dg)
      return se;
    eqlb_se_destroy(se);
    se = nullptr;
    check(eqlb_se_create(mesh->h, k, degree_dg, nrhs, stress ? 1 : 0, 0, &se));
    try
    {
      for (const auto& o : se_options)
        check(eqlb_se_set_option(se, o.first.c_str(), o.second));
      check(eqlb_se_set_boundary(se, facet_type.data(), boundary_values.empty() ? nullptr : boundary_values.data(),
                                 nullptr));
    }
    catch (...)
    {
      eqlb_se_destroy(se); // no handle without boundary data is kept
      se = nullptr;
      throw;
    }
    se_degree_dg = degree_dg;
    return se;
  }
  eqlb_ev_t* ev_handle(int degree_dg)
  {
    if (custom)
      throw std::runtime_error("reconstruct_fluxes_minimisation: the boundary data belongs to the discontinuous "
                               "(semi-explicit) flux space");
    if (ev && ev_degree_dg == degree_dg)
      return ev;
    eqlb_ev_destroy(ev);
    ev = nullptr;
    check(eqlb_ev_create_dg(mesh->h, k, degree_dg, nrhs, &ev));
    try
    {
      for (const auto& o : ev_options)
        check(eqlb_ev_set_option(ev, o.first.c_str(), o.second));
      if (!V->cell_dofs.empty())
        check(eqlb_ev_set_dofmap(ev, V->cell_dofs.data(), V->ndofs_user));
      if (!basis_C.empty())
      {
        // the boundary DOFs of this object are facet moments, i.e. hierarchic DOFs: the library converts them
        check(eqlb_ev_set_basis_transform(ev, basis_C.data(), basis_R.empty() ? nullptr : basis_R.data()));
        check(eqlb_ev_set_option(ev, "boundary_basis", 1));
      }
      check(eqlb_ev_set_boundary(ev, facet_type.data(), boundary_values.empty() ? nullptr : boundary_values.data(),
                                 nullptr));
    }
    catch (...)
    {
      eqlb_ev_destroy(ev); // no handle without boundary data is kept
      ev = nullptr;
      throw;
    }
    ev_degree_dg = degree_dg;
    return ev;
  }
  // Output basis of the conforming flux (eqlb_ev_set_basis_transform): C [k(k+2)]^2 from the hierarchic
  // reference coefficients to the target element's, R [k]^2 for the facet block of reflected facets.
  void set_basis_transform(const py::array_t<double, py::array::c_style | py::array::forcecast>& C,
                           const py::object& R)
  {
    if (custom)
      throw std::runtime_error("set_basis_transform: only for the conforming (minimisation) flux space");
    const int nrt = k * (k + 2);
    if (C.ndim() != 2 || C.shape(0) != nrt || C.shape(1) != nrt)
      throw std::runtime_error("set_basis_transform: C must be [k(k+2), k(k+2)]");
    basis_C.assign(C.data(), C.data() + (size_t)nrt * nrt);
    basis_R.clear();
    if (!R.is_none())
    {
      auto r = R.cast<py::array_t<double, py::array::c_style | py::array::forcecast>>();
      if (r.ndim() != 2 || r.shape(0) != k || r.shape(1) != k)
        throw std::runtime_error("set_basis_transform: R must be [k, k]");
      basis_R.assign(r.data(), r.data() + (size_t)k * k);
    }
    eqlb_ev_destroy(ev); // rebuilt with the new basis on the next call
    ev = nullptr;
    // (the options of the old handle go with it, except the one that decides whether the new one can be built)
    ev_options.erase(std::remove_if(ev_options.begin(), ev_options.end(),
                                    [](const std::pair<std::string, int>& o) { return o.first != "large_patches"; }),
                     ev_options.end());
  }
  void set_option(const std::string& key, int value)
  {
    // The option is checked at once - on the handle if there is one, else on a throw-away handle - and only a valid
    // one is kept (one entry per key) for handles created or rebuilt later.  "large_patches" acts in
    // eqlb_*_set_boundary, and so does "large_patches_stress" (SE handles only): an existing handle is dropped and
    // rebuilt with it on the next call.
    const bool rebuild = key == "large_patches" || key == "large_patches_stress";
    auto keep = [&](std::vector<std::pair<std::string, int>>& opts) {
      for (auto& o : opts)
        if (o.first == key)
        {
          o.second = value;
          return;
        }
      opts.emplace_back(key, value);
    };
    if (custom)
    {
      if (se)
        check(eqlb_se_set_option(se, key.c_str(), value));
      else
      {
        eqlb_se_t* tmp = nullptr;
        check(eqlb_se_create(mesh->h, k, k - 1, 1, 0, 0, &tmp));
        const int st = eqlb_se_set_option(tmp, key.c_str(), value);
        eqlb_se_destroy(tmp);
        check(st);
      }
      keep(se_options);
      if (se && rebuild)
      {
        eqlb_se_destroy(se);
        se = nullptr;
      }
    }
    else
    {
      if (ev)
        check(eqlb_ev_set_option(ev, key.c_str(), value));
      else
      {
        eqlb_ev_t* tmp = nullptr;
        check(eqlb_ev_create_dg(mesh->h, k, k - 1, 1, &tmp));
        const int st = eqlb_ev_set_option(tmp, key.c_str(), value);
        eqlb_ev_destroy(tmp);
        check(st);
      }
      keep(ev_options);
      if (ev && rebuild)
      {
        eqlb_ev_destroy(ev);
        ev = nullptr;
      }
    }
  }
};

int memspace_of(const std::vector<std::shared_ptr<Function>>& a, const std::vector<std::shared_ptr<Function>>& b,
                const std::vector<std::shared_ptr<Function>>& c)
{
  int ndev = 0, n = 0;
  for (const auto* l : {&a, &b, &c})
    for (const auto& f : *l)
    {
      if (!f)
        throw std::runtime_error("Equilibration: Input sizes does not match");
      ndev += f->on_device ? 1 : 0;
      ++n;
    }
  if (ndev != 0 && ndev != n)
    throw std::runtime_error("Equilibration: all Functions of a call must live in the same memory space");
  return ndev ? EQLB_MEM_DEVICE : EQLB_MEM_HOST;
}

void semiexplt(std::vector<std::shared_ptr<Function>>& flux_hdiv, std::vector<std::shared_ptr<Function>>& flux_dg,
               std::vector<std::shared_ptr<Function>>& rhs_dg, std::shared_ptr<BoundaryData> bd,
               bool reconstruct_stress, std::shared_ptr<Function> korn)
{
  // se/reconstruction.hpp:345-388
  if (!bd)
    throw std::runtime_error("Equilibration: Input sizes does not match");
  const size_t n = flux_hdiv.size();
  if (n == 0 || flux_dg.size() != n || rhs_dg.size() != n || (int)n != bd->nrhs)
    throw std::runtime_error("Equilibration: Input sizes does not match");
  const int mem = memspace_of(flux_hdiv, flux_dg, rhs_dg);
  const int k = bd->k;
  int degree_dg = -1;
  for (size_t i = 0; i < n; ++i)
  {
    const auto &Vh = flux_hdiv[i]->V, &Vg = flux_dg[i]->V, &Vf = rhs_dg[i]->V;
    if (Vh->family != "RT" || !Vh->discontinuous || Vh->degree != k || Vh->mesh != bd->mesh)
      throw std::runtime_error("Equilibration: flux_hdiv must live in the flux space of the boundary data");
    if (Vg->family != "DG" || Vf->family != "DG" || Vg->bs != 2 || Vf->bs != 1 || Vg->mesh != bd->mesh
        || Vf->mesh != bd->mesh)
      throw std::runtime_error("Equilibration: Input sizes does not match");
    if (Vg->degree != Vf->degree || Vg->degree > k - 1 || (degree_dg >= 0 && Vg->degree != degree_dg))
      throw std::runtime_error("Equilibration: Wrong polynomial degree of the projected RHS");
    degree_dg = Vg->degree;
  }
  if (reconstruct_stress)
  {
    if (n < 2)
      throw std::runtime_error("Stress equilibration: Specify all rows of stress tensor");
    if (k < 2)
      throw std::runtime_error("Stress equilibration: RT_k with k>1 required!");
  }
  eqlb_se_t* h = bd->se_handle(degree_dg, reconstruct_stress);
  std::vector<const double*> g(n), f(n);
  std::vector<double*> x(n);
  for (size_t i = 0; i < n; ++i)
  {
    g[i] = flux_dg[i]->data();
    f[i] = rhs_dg[i]->data();
    x[i] = flux_hdiv[i]->data();
  }
  {
    py::gil_scoped_release nogil;
    check(eqlb_se_equilibrate_lists(h, g.data(), f.data(), x.data(), mem, g_stream));
  }
  if (korn)
  {
    if (korn->V->family != "DG" || korn->V->degree != 0 || korn->V->bs != 1 || korn->on_device != (mem == EQLB_MEM_DEVICE))
      throw std::runtime_error("Equilibration: cells_kornconst must be a DG0 Function in the memory space of the call");
    py::gil_scoped_release nogil;
    check(eqlb_se_kornconst(h, korn->data(), mem, g_stream));
  }
}

void minimisation(const Form&, const Form&, const std::vector<std::shared_ptr<Form>>& l,
                  std::vector<std::shared_ptr<Function>>& flux_hdiv, std::shared_ptr<BoundaryData> bd)
{
  if (!bd || l.size() != flux_hdiv.size() || (int)l.size() != bd->nrhs || l.empty())
    throw std::runtime_error("Equilibration: Input sizes does not match");
  const size_t n = l.size();
  std::vector<std::shared_ptr<Function>> gs, fs;
  for (const auto& li : l)
  {
    // l_i = hat G_i . v + (hat f_i + grad hat . G_i) q  (FluxEqlbEV.py:129-134): coefficients [G_i, f_i]
    if (!li || li->coefficients.size() != 2)
      throw std::runtime_error("reconstruct_fluxes_minimisation: l[i] carries the coefficients [flux_dg_i, rhs_dg_i]");
    gs.push_back(li->coefficients[0]);
    fs.push_back(li->coefficients[1]);
  }
  const int mem = memspace_of(flux_hdiv, gs, fs);
  const int k = bd->k;
  // G_i, f_i in one DG_d, d <= k-1 (the kernels read DG_d directly)
  const int degree_dg = gs[0]->V->degree;
  for (size_t i = 0; i < n; ++i)
  {
    const auto &Vh = flux_hdiv[i]->V, &Vg = gs[i]->V, &Vf = fs[i]->V;
    if (Vh != bd->V && !(Vh->family == "RT" && !Vh->discontinuous && Vh->degree == k && Vh->mesh == bd->mesh))
      throw std::runtime_error("Equilibration: flux_hdiv must live in the flux space of the boundary data");
    if (Vg->family != "DG" || Vf->family != "DG" || Vg->bs != 2 || Vf->bs != 1 || Vg->degree != degree_dg
        || Vf->degree != degree_dg || degree_dg < 0 || degree_dg > k - 1 || Vg->mesh != bd->mesh
        || Vf->mesh != bd->mesh)
      throw std::runtime_error("Equilibration: Input sizes does not match");
  }
  eqlb_ev_t* h = bd->ev_handle(degree_dg);
  std::vector<const double*> g(n), f(n);
  std::vector<double*> x(n);
  for (size_t i = 0; i < n; ++i)
  {
    g[i] = gs[i]->data();
    f[i] = fs[i]->data();
    x[i] = flux_hdiv[i]->data();
  }
  py::gil_scoped_release nogil;
  check(eqlb_ev_equilibrate_lists(h, g.data(), f.data(), x.data(), mem, g_stream));
}

// base::local_solver (base/local_solver.hpp:38-187): a = (u, v) on the space of the solutions, l_i = (f_i, v)
void local_solver(std::vector<std::shared_ptr<Function>>& sol, const Form&, const std::vector<std::shared_ptr<Form>>& l)
{
  if (sol.empty() || sol.size() != l.size())
    throw std::runtime_error("Local solver: Input sizes does not match");
  for (size_t i = 0; i < sol.size(); ++i)
  {
    const auto& u = sol[i];
    if (!u || !l[i] || !l[i]->has_points || u->V->family != "DG")
      throw std::runtime_error("Local solver: DG solutions and forms with point values expected");
    const auto& m = u->V->mesh;
    const int nq = (int)l[i]->qweights.size(), bs = u->V->bs;
    if (l[i]->qvalues.size() != (py::ssize_t)m->ncells * nq * bs)
      throw std::runtime_error("Local solver: Input sizes does not match");
    double* out = u->data();
    const double *qp = l[i]->qpoints.data(), *qw = l[i]->qweights.data(), *qv = l[i]->qvalues.data();
    if (u->on_device)
      throw std::runtime_error("Local solver: host Functions expected (point values are host arrays)");
    py::gil_scoped_release nogil;
    check(eqlb_project_dg(m->h, u->V->degree, bs, 1, nq, qp, qw, qv, out, EQLB_MEM_HOST, g_stream));
  }
}

// ---- multi-GPU: reverse halo over RCCL through the C ABI (include/eqlb.h: eqlb_halo_*, eqlb_rccl_*) --------------
// No counterpart in the reference module (its node loop covers the owned nodes of one process,
// cpp/dolfinx_eqlb/se/reconstruction.hpp:90); this is the C++ host's own multi-GPU path: one process per GPU, a
// communicator made from a unique id the caller distributes (MPI where DOLFINx runs), one call per sweep.
struct RcclComm
{
  void* comm = nullptr;
  int nranks = 0, rank = 0;
  RcclComm(py::bytes unique_id, int nranks_, int rank_) : nranks(nranks_), rank(rank_)
  {
    const std::string id = unique_id;
    if (id.size() != 128)
      throw std::runtime_error("RcclComm: the unique id has 128 bytes");
    check(eqlb_rccl_comm_create(id.data(), nranks, rank, &comm));
  }
  ~RcclComm() { eqlb_rccl_comm_destroy(comm); }
  RcclComm(const RcclComm&) = delete;
  RcclComm& operator=(const RcclComm&) = delete;
};

struct HaloExchange
{
  eqlb_halo_t* h = nullptr;
  int64_t nentries;
  int nrhs, width;
  // send / recv: {peer rank: int64 index array} - rows (of `width` doubles) that leave to / arrive from the peer
  HaloExchange(int nrhs_, int width_, int64_t nentries_, std::map<int, carray<int64_t>> send,
               std::map<int, carray<int64_t>> recv)
      : nentries(nentries_), nrhs(nrhs_), width(width_)
  {
    std::vector<int32_t> peers;
    for (auto& kv : send)
      peers.push_back(kv.first);
    for (auto& kv : recv)
      if (!send.count(kv.first))
        peers.push_back(kv.first);
    std::sort(peers.begin(), peers.end());
    std::vector<const int64_t*> si, ri;
    std::vector<int64_t> ns, nr;
    for (int32_t q : peers)
    {
      auto s_ = send.find(q);
      auto r_ = recv.find(q);
      si.push_back(s_ != send.end() ? s_->second.data() : nullptr);
      ns.push_back(s_ != send.end() ? (int64_t)s_->second.size() : 0);
      ri.push_back(r_ != recv.end() ? r_->second.data() : nullptr);
      nr.push_back(r_ != recv.end() ? (int64_t)r_->second.size() : 0);
    }
    check(eqlb_halo_create(nrhs, width, nentries, (int32_t)peers.size(), peers.data(), si.data(), ns.data(),
                           ri.data(), nr.data(), &h));
  }
  ~HaloExchange() { eqlb_halo_destroy(h); }
  HaloExchange(const HaloExchange&) = delete;
  HaloExchange& operator=(const HaloExchange&) = delete;
  void reduce_ptr(RcclComm& c, uintptr_t x)
  {
    if (!x)
      throw std::runtime_error("HaloExchange.reduce: null device pointer");
    check(eqlb_halo_reduce_plan(h, c.comm, reinterpret_cast<double*>(x), g_stream));
  }
  void reduce(RcclComm& c, std::vector<std::shared_ptr<Function>> fs)
  {
    // the right-hand sides of one call share a halo: consecutive device blocks of one array
    if ((int)fs.size() != nrhs || !fs[0] || !fs[0]->on_device)
      throw std::runtime_error("HaloExchange.reduce: nrhs device-memory Functions (Function.from_device) expected");
    for (int r = 0; r < nrhs; ++r)
      if (!fs[r] || !fs[r]->on_device || fs[r]->size() != nentries * width
          || fs[r]->dev != fs[0]->dev + (uintptr_t)r * nentries * width * sizeof(double))
        throw std::runtime_error("HaloExchange.reduce: the Functions must be consecutive blocks of one device array");
    reduce_ptr(c, fs[0]->dev);
  }
  py::tuple bytes() const
  {
    int64_t s = 0, r = 0;
    check(eqlb_halo_bytes(h, &s, &r));
    return py::make_tuple(s, r);
  }
};

} // namespace

PYBIND11_MODULE(_cpp, m)
{
  m.doc() = "dolfinx_eqlb_amd: MI355X-native patch-local flux equilibration - interface of dolfinx_eqlb.cpp";

  py::class_<Mesh, std::shared_ptr<Mesh>>(m, "Mesh", "Flat triangle mesh on the device (stand-in of dolfinx.mesh.Mesh)")
      .def(py::init<carray<double>, carray<int32_t>, carray<int32_t>, carray<int32_t>, carray<int32_t>,
                    carray<int32_t>, carray<int32_t>, carray<int32_t>, carray<int32_t>, carray<int32_t>,
                    carray<uint8_t>>(),
           py::arg("x"), py::arg("cell_nodes"), py::arg("cell_facets"), py::arg("facet_nodes"),
           py::arg("facet_cells_offsets"), py::arg("facet_cells"), py::arg("node_cells_offsets"),
           py::arg("node_cells"), py::arg("node_facets_offsets"), py::arg("node_facets"), py::arg("facet_perm"))
      .def_static("from_cells", &Mesh::from_cells, py::arg("x"), py::arg("cell_nodes"),
                  "Mesh from coordinates [nnodes, 2 or 3] and cells [ncells, 3]: the connectivity is built on the device")
      .def("boundary_facets", &Mesh::boundary_facets, "ids of the facets with one cell, ascending")
      .def("find_facets", &Mesh::find_facets, py::arg("pairs"),
           "facet id of every node pair [npairs, 2] (either order), -1 where the pair is no edge")
      .def("refine", &Mesh::refine, py::arg("marked"), py::arg("keep_plan") = false,
           "(Mesh, parent_cell, node_parent_facet, parent_facet) of the mesh refined at the marked cells by longest-edge "
           "closure and bisection, on the device; keep_plan=True appends a Transfer that prolongs host arrays")
      .def("lagrange_dofmap", &Mesh::lagrange_dofmap, py::arg("p"),
           "(cell_dofs [ncells, nd_p] int32, ndofs) of the conforming P_p space, 1 <= p <= 4")
      .def_property_readonly("x", [](const Mesh& s) {
        return py::array_t<double>({(py::ssize_t)s.nnodes, (py::ssize_t)3}, s.x.data());
      })
      .def_property_readonly("cell_nodes", [](const Mesh& s) {
        return py::array_t<int32_t>({(py::ssize_t)s.ncells, (py::ssize_t)3}, s.cell_nodes.data());
      })
      .def_readonly("nnodes", &Mesh::nnodes)
      .def_readonly("ncells", &Mesh::ncells)
      .def_readonly("nfacets", &Mesh::nfacets)
      .def_property_readonly("max_patch_cells", [](const Mesh& s) { return eqlb_mesh_max_patch_cells(s.h); });

  py::class_<Transfer, std::shared_ptr<Transfer>>(m, "Transfer",
                                                  "Open plan of Mesh.refine(..., keep_plan=True): carries P_p solutions "
                                                  "and DG data from the old mesh to the refined one")
      .def("prolong", &Transfer::prolong, py::arg("p"), py::arg("u"), py::arg("cell_dofs") = py::none(),
           py::arg("cell_dofs2") = py::none(), py::arg("bs") = 1, py::arg("ndofs2") = py::none(),
           "u [nrhs, ndofs*bs] in P_p on the old mesh -> [nrhs, ndofs2*bs] on the refined mesh")
      .def("prolong_dg", &Transfer::prolong_dg, py::arg("degree"), py::arg("values"), py::arg("bs") = 1,
           "DG_degree values [nrhs, ncells*nd*bs] -> [nrhs, ncells2*nd*bs]")
      .def("facet_types", &Transfer::facet_types, py::arg("facet_type"),
           "facet types [nrhs, nfacets] of the old mesh -> [nrhs, nfacets2]: the type of the parent facet, 0 without one")
      .def("child_facets", &Transfer::child_facets, py::arg("facets"),
           "old facet ids [nlist] -> children [nlist, 2] on the refined mesh, (f2, -1) for a facet that is not bisected")
      .def("prolong_flux_bc", &Transfer::prolong_flux_bc, py::arg("k"), py::arg("boundary_values"), py::arg("facets2"),
           "flux-BC table [nrhs, ncells*k(k+2)] of the old mesh -> facet DOFs [nrhs, nlist, k] of the listed boundary "
           "facets of the refined mesh")
      .def_readonly("coarse", &Transfer::coarse)
      .def_readonly("fine", &Transfer::fine);

  py::class_<PrimalPoisson, std::shared_ptr<PrimalPoisson>>(
      m, "PrimalPoisson", "-div(coeff grad u) = f on the P_p space of the mesh (numbering of Mesh.lagrange_dofmap): "
                          "matrix-free operator, load, residual and Jacobi-preconditioned CG on the device")
      .def(py::init<std::shared_ptr<Mesh>, int, py::object>(), py::arg("mesh"), py::arg("p"),
           py::arg("coeff") = py::none())
      .def("set_dirichlet", &PrimalPoisson::set_dirichlet, py::arg("facets"),
           "fixed are the vertex and facet DOFs of the listed facets; a repeated call replaces the mask")
      .def("set_reaction", &PrimalPoisson::set_reaction, py::arg("c") = 0.0, py::arg("cell_c") = py::none(),
           "the operator gains + c u: cell_c [ncells] where given, else the scalar; c = 0 without an array switches "
           "the term off; Multilevel.set_coarse(True) has to be called again afterwards")
      .def("set_diffusion", &PrimalPoisson::set_diffusion, py::arg("cell_D") = py::none(),
           "the operator becomes -div(coeff D grad u): cell_D [ncells][3] = (d00, d01, d11), symmetric positive "
           "definite per cell; None switches the term off; Multilevel.set_coarse(True) has to be called again afterwards")
      .def("set_robin", &PrimalPoisson::set_robin, py::arg("facets"), py::arg("alpha") = 1.0,
           py::arg("facet_alpha") = py::none(),
           "the operator gains int alpha u v over the listed boundary facets: facet_alpha [nlist] where given, else the "
           "scalar; an empty list switches the term off; Multilevel.set_coarse(True) has to be called again afterwards")
      .def("robin_weights", &PrimalPoisson::robin_weights, "w_f = alpha_f |E_f| [nlist] in the order of the list")
      .def("robin_flux", &PrimalPoisson::robin_flux, py::arg("u"), py::arg("s"), py::arg("u_ext") = py::none(),
           "out [nlist, nq] = alpha_i (u_h(x_q) - u_ext[i][q]) on the Robin list at the facet parameters s: the point "
           "values of the flux condition that update_flux_bc takes with vector = False")
      .def("load", &PrimalPoisson::load, py::arg("degree_dg"), py::arg("rhs_dg"), py::arg("b_extra") = py::none(),
           "b [ndofs] from DG_d nodal values rhs_dg [ncells*nd_d], + b_extra where given")
      .def("apply", &PrimalPoisson::apply, py::arg("u"), py::arg("masked") = false, "y = A u; masked: 0 on the fixed rows")
      .def("diagonal", &PrimalPoisson::diagonal)
      .def("matrix", &PrimalPoisson::matrix, py::arg("eliminate") = false,
           "(indptr int64 [n + 1], indices int32 [nnz], values [nnz]): the operator as CSR, assembled on the device; "
           "eliminate: P A P + (I - P) on the mask; scipy.sparse.csr_matrix((values, indices, indptr), shape=(n, n))")
      .def("matrix_values", &PrimalPoisson::matrix_values, py::arg("eliminate") = false,
           "values [nnz] from the coefficients, the terms and the mask the handle has now, on the pattern as it stands")
      .def("matrix_release", &PrimalPoisson::matrix_release, "frees the cached pattern; the next matrix() builds it again")
      .def("residual", &PrimalPoisson::residual, py::arg("b"), py::arg("u"),
           "(r, || r ||_2, nb): r = b - A u with 0 on the fixed rows")
      .def("solve", &PrimalPoisson::solve, py::arg("b"), py::arg("u"), py::arg("rtol") = 1e-8, py::arg("atol") = 0.0,
           py::arg("maxit") = 10000, "(u, info): PCG from the start u, whose fixed rows hold the Dirichlet values")
      .def("apply_many", &PrimalPoisson::apply_many, py::arg("U"), py::arg("masked") = false,
           "Y [nrhs][ndofs]: row c is apply(U[c]), bit for bit, in one call")
      .def("solve_many", &PrimalPoisson::solve_many, py::arg("B"), py::arg("U"), py::arg("rtol") = 1e-8,
           py::arg("atol") = 0.0, py::arg("maxit") = 10000,
           "(U, infos): nrhs systems in one call; row c and infos[c] are solve(B[c], U[c]), bit for bit")
      .def_readonly("mesh", &PrimalPoisson::mesh)
      .def_readonly("p", &PrimalPoisson::p)
      .def_readonly("ndofs", &PrimalPoisson::ndofs);

  py::class_<PrimalElasticity, std::shared_ptr<PrimalElasticity>>(
      m, "PrimalElasticity", "-div(2 eps(u) + pi_1 div(u) I) = f on [P_p]^2 of the mesh (scalar numbering of "
                             "Mesh.lagrange_dofmap, blocked x[2 dof + r]): matrix-free operator, load, residual and "
                             "Jacobi-preconditioned CG on the device")
      .def(py::init<std::shared_ptr<Mesh>, int, double, py::object>(), py::arg("mesh"), py::arg("p"),
           py::arg("pi_1") = 1.0, py::arg("cell_pi1") = py::none())
      .def("set_dirichlet", &PrimalElasticity::set_dirichlet, py::arg("facets0"), py::arg("facets1"),
           "fixed are the rows 2 dof + r of the vertex and facet DOFs of the facets listed for component r; a repeated "
           "call replaces the mask")
      .def("set_reaction", &PrimalElasticity::set_reaction, py::arg("c") = 0.0, py::arg("cell_c") = py::none(),
           "the operator gains + c u: cell_c [ncells] where given, else the scalar; c = 0 without an array switches "
           "the term off; Multilevel.set_coarse(True) has to be called again afterwards")
      .def("set_shear", &PrimalElasticity::set_shear, py::arg("mu") = 1.0, py::arg("cell_mu") = py::none(),
           "the stress becomes mu (2 eps(u) + pi_1 div(u) I): cell_mu [ncells] where given, else the scalar, mu > 0; "
           "mu = 1 without an array switches the term off; the reaction term is not scaled; "
           "Multilevel.set_coarse(True) has to be called again afterwards")
      .def("set_springs", &PrimalElasticity::set_springs, py::arg("facets"), py::arg("k") = 1.0,
           py::arg("facet_k") = py::none(),
           "the operator gains int_E v^T K u over the listed boundary facets: facet_k [nlist, 3] = (k00, k01, k11) where "
           "given, else k I; an empty list switches the term off; Multilevel.set_coarse(True) has to be called again "
           "afterwards")
      .def("spring_count", &PrimalElasticity::spring_count, "the number of listed facets of the spring term")
      .def("spring_weights", &PrimalElasticity::spring_weights,
           "Kw_f = |E_f| (k00, k01, k11) [nlist, 3] in the order of the list")
      .def("spring_flux", &PrimalElasticity::spring_flux, py::arg("u"), py::arg("s"), py::arg("u_ext") = py::none(),
           "out [2, nlist, nq] = K_i (u_h(x_q) - u_ext[.][i][q]) on the spring list at the facet parameters s: row r "
           "holds the point values of the flux condition of stress row r (update_flux_bc with vector = False)")
      .def("load", &PrimalElasticity::load, py::arg("degree_dg"), py::arg("rhs_dg"), py::arg("b_extra") = py::none(),
           "b [2 ndofs] from DG_d nodal values rhs_dg [2, ncells*nd_d], + b_extra where given")
      .def("apply", &PrimalElasticity::apply, py::arg("u"), py::arg("masked") = false,
           "y = A u; masked: 0 on the fixed rows")
      .def("diagonal", &PrimalElasticity::diagonal)
      .def("matrix", &PrimalElasticity::matrix, py::arg("eliminate") = false,
           "(indptr int64 [n + 1], indices int32 [nnz], values [nnz]): the operator as CSR, assembled on the device; "
           "eliminate: P A P + (I - P) on the mask; scipy.sparse.csr_matrix((values, indices, indptr), shape=(n, n))")
      .def("matrix_values", &PrimalElasticity::matrix_values, py::arg("eliminate") = false,
           "values [nnz] from the coefficients, the terms and the mask the handle has now, on the pattern as it stands")
      .def("matrix_release", &PrimalElasticity::matrix_release, "frees the cached pattern; the next matrix() builds it again")
      .def("residual", &PrimalElasticity::residual, py::arg("b"), py::arg("u"),
           "(r, || r ||_2, nb): r = b - A u with 0 on the fixed rows")
      .def("solve", &PrimalElasticity::solve, py::arg("b"), py::arg("u"), py::arg("rtol") = 1e-8, py::arg("atol") = 0.0,
           py::arg("maxit") = 10000, "(u, info): PCG from the start u, whose fixed rows hold the Dirichlet values")
      .def_readonly("mesh", &PrimalElasticity::mesh)
      .def_readonly("p", &PrimalElasticity::p)
      .def_readonly("ndofs", &PrimalElasticity::ndofs);

  m.def("csr_apply", &csr_apply, py::arg("indptr"), py::arg("indices"), py::arg("values"), py::arg("x"),
        "y = A x for a CSR matrix, on the device: the row sum in ascending positions, each product and sum rounded singly");

  py::class_<Multilevel, std::shared_ptr<Multilevel>>(
      m, "Multilevel", "Multilevel preconditioner (BPX) over the levels of an adaptive loop: solvers coarsest first (all "
                       "PrimalPoisson or all PrimalElasticity), transfers[l] the Transfer of Mesh.refine(..., "
                       "keep_plan=True) between level l and l + 1 (eqlb_hierarchy_*)")
      .def(py::init<py::list, py::list, bool, bool>(), py::arg("solvers"), py::arg("transfers"),
           py::arg("local") = false, py::arg("coarse") = false)
      .def_property("coarse", [](const Multilevel& self) { return self.coarse; }, &Multilevel::set_coarse,
                    "exact solve on the free rows of level 0 by a dense LDL^T factor (a snapshot: set it again after "
                    "set_dirichlet or a new coefficient on level 0)")
      .def_property_readonly("coarse_rows", &Multilevel::coarse_rows, "the free rows of level 0 the factor was formed on")
      .def("coarse_factor", &Multilevel::coarse_factor, "(rows int32 [n], d [n], W [n][n]): the factor of level 0")
      .def_property("local", [](const Multilevel& self) { return self.local; }, &Multilevel::set_local,
                    "local smoothing: a level l >= 1 smooths only the rows whose basis function is new or changed there")
      .def("active", &Multilevel::active, py::arg("level"), "bool [bs ndofs_level]: the rows smoothed on `level`")
      .def("active_count", &Multilevel::active_count, py::arg("level"), "the number of rows smoothed on `level`")
      .def("restrict", &Multilevel::restrict, py::arg("level"), py::arg("r"), py::arg("masked") = true,
           "r [level + 1] -> P^T r [level]; masked: 0 on the fixed rows of the coarse level")
      .def("precondition", &Multilevel::precondition, py::arg("r"), "z = M r on the finest level")
      .def("solve", &Multilevel::solve, py::arg("b"), py::arg("u"), py::arg("rtol") = 1e-8, py::arg("atol") = 0.0,
           py::arg("maxit") = 10000, "(u, info): the CG of the finest solver with the multilevel preconditioner")
      .def("precondition_many", &Multilevel::precondition_many, py::arg("R"),
           "Z [nrhs][n]: row c is precondition(R[c]), bit for bit, in one call (Poisson handles only)")
      .def("solve_many", &Multilevel::solve_many, py::arg("B"), py::arg("U"), py::arg("rtol") = 1e-8,
           py::arg("atol") = 0.0, py::arg("maxit") = 10000,
           "(U, infos): nrhs systems in one call; row c and infos[c] are solve(B[c], U[c]) (Poisson handles only)")
      .def_readonly("nlevels", &Multilevel::nlevels)
      .def_readonly("bs", &Multilevel::bs);

  py::class_<FunctionSpace, std::shared_ptr<FunctionSpace>>(m, "FunctionSpace")
      .def(py::init<std::shared_ptr<Mesh>, std::string, int, int, bool>(), py::arg("mesh"), py::arg("family"),
           py::arg("degree"), py::arg("bs") = 1, py::arg("discontinuous") = true)
      .def("set_dofmap", &FunctionSpace::set_dofmap, py::arg("cell_dofs"), py::arg("ndofs"))
      .def_readonly("mesh", &FunctionSpace::mesh)
      .def_readonly("family", &FunctionSpace::family)
      .def_readonly("degree", &FunctionSpace::degree)
      .def_readonly("bs", &FunctionSpace::bs)
      .def_readonly("discontinuous", &FunctionSpace::discontinuous)
      .def_property_readonly("ndofs", &FunctionSpace::ndofs);

  py::class_<Function, std::shared_ptr<Function>>(m, "Function")
      .def(py::init<std::shared_ptr<FunctionSpace>>(), py::arg("V"))
      .def(py::init<std::shared_ptr<FunctionSpace>, py::array_t<double>>(), py::arg("V"), py::arg("array"))
      .def_static("from_device", &Function::from_device, py::arg("V"), py::arg("device_ptr"))
      .def_readonly("function_space", &Function::V)
      .def_readonly("on_device", &Function::on_device)
      .def_property_readonly("device_ptr", [](const Function& f) { return f.dev; })
      .def_property_readonly("array", [](Function& f) -> py::object {
        if (f.on_device)
          throw std::runtime_error("Function.array: the values live on the device");
        return f.host;
      });

  py::class_<Constant, std::shared_ptr<Constant>>(m, "Constant").def(py::init<carray<double>>(), py::arg("value"));

  py::class_<Form, std::shared_ptr<Form>>(m, "Form")
      .def(py::init<std::vector<std::shared_ptr<Function>>>(), py::arg("coefficients") = std::vector<std::shared_ptr<Function>>{})
      .def_static("from_point_values", &Form::from_point_values, py::arg("qpoints"), py::arg("qweights"),
                  py::arg("qvalues"));

  // ---- boundary conditions (wrappers.cpp:140-257) ----
  py::class_<FluxBC, std::shared_ptr<FluxBC>>(m, "FluxBC", "FluxBC object")
      .def(py::init([](std::shared_ptr<FunctionSpace> V, const std::vector<int32_t>& facets, uintptr_t kernel_ptr,
                       int n_bceval_per_fct, std::vector<std::shared_ptr<Function>> coefficients,
                       std::vector<int> positions, std::vector<std::shared_ptr<Constant>> constants) {
             return std::make_shared<FluxBC>(V, facets, kernel_ptr, n_bceval_per_fct, 0, false, coefficients,
                                             positions, constants);
           }),
           py::arg("function_space"), py::arg("facets"), py::arg("pointer_boundary_kernel"),
           py::arg("nevals_per_fct"), py::arg("coefficients"), py::arg("position_of_coefficients"),
           py::arg("constants"))
      .def(py::init([](std::shared_ptr<FunctionSpace> V, const std::vector<int32_t>& facets, uintptr_t kernel_ptr,
                       int n_bceval_per_fct, int quadrature_degree,
                       std::vector<std::shared_ptr<Function>> coefficients, std::vector<int> positions,
                       std::vector<std::shared_ptr<Constant>> constants) {
             return std::make_shared<FluxBC>(V, facets, kernel_ptr, n_bceval_per_fct, quadrature_degree, true,
                                             coefficients, positions, constants);
           }),
           py::arg("function_space"), py::arg("facets"), py::arg("pointer_boundary_kernel"),
           py::arg("nevals_per_fct"), py::arg("quadrature_degree"), py::arg("coefficients"),
           py::arg("position_of_coefficients"), py::arg("constants"))
      .def_property_readonly("quadrature_degree", [](const FluxBC& b) { return b.qdegree; });

  py::class_<BoundaryData, std::shared_ptr<BoundaryData>>(m, "BoundaryData", py::dynamic_attr(), "BoundaryData object")
      .def(py::init([](std::vector<std::vector<std::shared_ptr<FluxBC>>>& list_bcs,
                       std::vector<std::shared_ptr<Function>>& boundary_flux, std::shared_ptr<FunctionSpace> V,
                       bool rtflux_is_custom, int quadrature_degree,
                       const std::vector<std::vector<int32_t>>& fct_esntbound_prime, bool reconstruct_stress) {
             return std::make_shared<BoundaryData>(list_bcs, boundary_flux, V, rtflux_is_custom, quadrature_degree,
                                                   fct_esntbound_prime, reconstruct_stress);
           }),
           py::arg("list_of_bcs"), py::arg("list_of_boundary_fluxes"), py::arg("V_flux_hdiv"),
           py::arg("rtflux_is_custom"), py::arg("quadrature_degree"), py::arg("list_bfcts_prime"),
           py::arg("reconstruct_stress"))
      .def("set_basis_transform", &BoundaryData::set_basis_transform, py::arg("C"), py::arg("R") = py::none(),
           "Output basis of the conforming flux: y_cell = C c_cell, R on the facet block of reflected facets")
      .def("update", &BoundaryData::update,
           "Evaluate the flux BCs again (same facets, new values) and push them to the device handle in place")
      .def("set_option", &BoundaryData::set_option, py::arg("key"), py::arg("value"),
           "Integer options of the device handle (eqlb_se_set_option / eqlb_ev_set_option)")
      .def_property_readonly("facet_type", [](const BoundaryData& b) {
        py::array_t<int8_t> a({(py::ssize_t)b.nrhs, (py::ssize_t)b.mesh->nfacets});
        std::copy(b.facet_type.begin(), b.facet_type.end(), a.mutable_data());
        return a;
      });

  // ---- local solvers (wrappers.cpp:52-80): one kernel, the exact inverse of the reference mass matrix ----
  for (const char* name : {"local_solver_lu", "local_solver_cholesky", "local_solver_cg"})
    m.def(name, &local_solver, py::arg("solution"), py::arg("a"), py::arg("l"),
          "Cell-local projection (base/local_solver.hpp:38-187) on the device");

  // ---- equilibration (wrappers.cpp:82-137) ----
  m.def("reconstruct_fluxes_minimisation", &minimisation, py::arg("a"), py::arg("l_pen"), py::arg("l"),
        py::arg("flux_hdiv"), py::arg("boundary_data"),
        "Local equilibration of H(div) conforming fluxes, solving patch-wise, constrained minimisation problems.");
  m.def(
      "reconstruct_fluxes_semiexplt",
      [](std::vector<std::shared_ptr<Function>>& flux_hdiv, std::vector<std::shared_ptr<Function>>& flux_dg,
         std::vector<std::shared_ptr<Function>>& rhs_dg, std::shared_ptr<BoundaryData> bd, bool reconstruct_stress)
      { semiexplt(flux_hdiv, flux_dg, rhs_dg, bd, reconstruct_stress, nullptr); },
      py::arg("flux_hdiv"), py::arg("flux_dg"), py::arg("rhs_dg"), py::arg("boundary_data"),
      py::arg("reconstruct_stress"),
      "Local equilibration of H(div) conforming fluxes, using an explicit determination of the fluxes followed by "
      "a minimisation on a reduced space; reconstruct_stress: weak symmetry of the first gdim rows.");
  m.def(
      "reconstruct_fluxes_semiexplt_with_kornconst",
      [](std::vector<std::shared_ptr<Function>>& flux_hdiv, std::vector<std::shared_ptr<Function>>& flux_dg,
         std::vector<std::shared_ptr<Function>>& rhs_dg, std::shared_ptr<BoundaryData> bd, bool reconstruct_stress,
         std::shared_ptr<Function> cells_kornconst)
      {
        if (!cells_kornconst)
          throw std::runtime_error("Equilibration: Input sizes does not match");
        semiexplt(flux_hdiv, flux_dg, rhs_dg, bd, reconstruct_stress, cells_kornconst);
      },
      py::arg("flux_hdiv"), py::arg("flux_dg"), py::arg("rhs_dg"), py::arg("boundary_data"),
      py::arg("reconstruct_stress"), py::arg("cells_kornconst"),
      "As reconstruct_fluxes_semiexplt; upper bounds of the cells' squared Korn constants are accumulated.");

  // ---- helpers without a counterpart in the reference module ----
  m.def("facet_quadrature", [](int degree) {
    std::vector<double> s, w;
    facet_rule(degree, s, w);
    return py::make_tuple(py::array_t<double>(s.size(), s.data()), py::array_t<double>(w.size(), w.data()));
  }, py::arg("degree"), "Gauss rule on [0, 1] used for flux BCs (requires_projection: `quadrature_degree`)");
  m.def("interpolation_quadrature_degree", &interpolation_degree, py::arg("degree_flux"),
        "Degree of the facet rule that stands for the element's interpolation points (no projection)");
  // ---- multi-GPU (no counterpart in the reference module) ----
  m.def("rccl_unique_id", []() {
    char id[128];
    check(eqlb_rccl_get_unique_id(id));
    return py::bytes(id, 128);
  }, "ncclUniqueId (128 bytes) for RcclComm: made on one rank, distributed by the caller");
  py::class_<RcclComm, std::shared_ptr<RcclComm>>(m, "RcclComm", "RCCL communicator (ncclCommInitRank through the C ABI)")
      .def(py::init<py::bytes, int, int>(), py::arg("unique_id"), py::arg("nranks"), py::arg("rank"))
      .def_readonly("nranks", &RcclComm::nranks)
      .def_readonly("rank", &RcclComm::rank);
  py::class_<HaloExchange, std::shared_ptr<HaloExchange>>(
      m, "HaloExchange", "Reverse halo of the node-ownership decomposition: ghost rows -> owner, added there")
      .def(py::init<int, int, int64_t, std::map<int, carray<int64_t>>, std::map<int, carray<int64_t>>>(),
           py::arg("nrhs"), py::arg("width"), py::arg("nentries"), py::arg("send"), py::arg("recv"))
      .def("reduce", &HaloExchange::reduce, py::arg("comm"), py::arg("flux_hdiv"),
           "pack + clear, grouped ncclSend / ncclRecv, unpack-add on the stream of set_stream")
      .def("reduce_ptr", &HaloExchange::reduce_ptr, py::arg("comm"), py::arg("device_pointer"))
      .def("bytes", &HaloExchange::bytes, "(bytes sent, bytes received) per reduction");
  m.def("set_stream", [](uintptr_t s) { g_stream = reinterpret_cast<void*>(s); }, py::arg("stream"),
        "hipStream_t used by calls on device-memory Functions (0: default stream)");
  m.def(
      "primal_value_dg",
      [](std::shared_ptr<Mesh> mesh, int p, int degree_dg, carray<int32_t> cell_dofs, darray u, py::object coeff,
         py::object op) {
        if (p < 1 || p > 4 || degree_dg < 0 || degree_dg > 3)
          throw std::runtime_error("primal_value_dg: degrees outside 1 ... 4, 0 ... 3");
        const py::ssize_t ndp = (p + 1) * (p + 2) / 2, nd = (degree_dg + 1) * (degree_dg + 2) / 2;
        const py::ssize_t nrhs = u.ndim() == 2 ? u.shape(0) : 1;
        const char* what = "primal_value_dg: Input sizes does not match";
        const OptArray kc = opt_array(coeff, mesh->ncells, what), t = opt_array(op, nd * ndp, what);
        if (cell_dofs.size() != (py::ssize_t)mesh->ncells * ndp || u.size() == 0 || u.size() % nrhs)
          throw std::runtime_error(what);
        darray out({nrhs, (py::ssize_t)mesh->ncells * nd});
        check(eqlb_primal_value_dg(mesh->h, p, degree_dg, (int32_t)nrhs, cell_dofs.data(), u.size() / nrhs, u.data(),
                                   kc.p, t.p, out.mutable_data(), EQLB_MEM_HOST, nullptr));
        return out;
      },
      py::arg("mesh"), py::arg("p"), py::arg("degree_dg"), py::arg("cell_dofs"), py::arg("u"),
      py::arg("coeff") = py::none(), py::arg("op") = py::none(),
      "[nrhs, ncells*nd_d]: the DG_d DOFs of coeff Pi_d u_h for u_h in P_p (eqlb_primal_value_dg); coeff [ncells] or "
      "None, op [nd_d, nd_p] replaces the built-in table");
  m.def(
      "primal_flux_dg",
      [](std::shared_ptr<Mesh> mesh, int p, int degree_dg, carray<int32_t> cell_dofs, darray u, py::object coeff,
         py::object op, py::object cell_D) {
        if (p < 1 || p > 4 || degree_dg < 0 || degree_dg > 3)
          throw std::runtime_error("primal_flux_dg: degrees outside 1 ... 4, 0 ... 3");
        const py::ssize_t ndp = (p + 1) * (p + 2) / 2, nd = (degree_dg + 1) * (degree_dg + 2) / 2;
        const py::ssize_t nrhs = u.ndim() == 2 ? u.shape(0) : 1;
        const char* what = "primal_flux_dg: Input sizes does not match";
        const OptArray kc = opt_array(coeff, mesh->ncells, what), t = opt_array(op, 2 * nd * ndp, what),
                       kd = opt_array(cell_D, (py::ssize_t)mesh->ncells * 3, what);
        if (cell_dofs.size() != (py::ssize_t)mesh->ncells * ndp || u.size() == 0 || u.size() % nrhs)
          throw std::runtime_error(what);
        darray out({nrhs, (py::ssize_t)mesh->ncells * nd * 2});
        if (!kd.p)
          check(eqlb_primal_flux_dg(mesh->h, p, degree_dg, (int32_t)nrhs, cell_dofs.data(), u.size() / nrhs, u.data(),
                                    kc.p, t.p, out.mutable_data(), EQLB_MEM_HOST, nullptr));
        else
          check(eqlb_primal_flux_dg_tensor(mesh->h, p, degree_dg, (int32_t)nrhs, cell_dofs.data(), u.size() / nrhs,
                                           u.data(), kc.p, kd.p, t.p, out.mutable_data(), EQLB_MEM_HOST, nullptr));
        return out;
      },
      py::arg("mesh"), py::arg("p"), py::arg("degree_dg"), py::arg("cell_dofs"), py::arg("u"),
      py::arg("coeff") = py::none(), py::arg("op") = py::none(), py::arg("cell_D") = py::none(),
      "[nrhs, ncells*nd_d*2]: the DG_d^2 DOFs of -coeff grad(u_h) for u_h in P_p (eqlb_primal_flux_dg), or of "
      "-coeff D grad(u_h) with cell_D [ncells][3] = (d00, d01, d11) (eqlb_primal_flux_dg_tensor); coeff [ncells] or "
      "None, op [2, nd_d, nd_p] replaces the built-in table");
  m.def("device_count", &eqlb_device_count);
  m.def("synchronize_and_check", [](std::shared_ptr<BoundaryData> bd) {
    if (bd->se)
      check(eqlb_se_check_status(bd->se, g_stream));
    if (bd->ev)
      check(eqlb_ev_check_status(bd->ev, g_stream));
  }, py::arg("boundary_data"), "Wait for the stream of device-memory calls and raise if a patch system was singular");
}
