// The planner of eqlb_se_set_boundary (dolfinx_eqlb_amd/csrc/eqlb_boundary_plan.h) on a mesh and a facet-type table
// read from a text file: prints the plan, or the code and the text of the refusal.
//
//   c++ -O1 -g -std=c++17 [-fsanitize=address,undefined] tools/boundary_plan_emul.cpp -o boundary_plan_emul
//   ./boundary_plan_emul case.txt
//
// No GPU, no HIP.  The input is a list of integers (tests/test_boundary_plan_host.py writes it):
//
//   nnodes ncells nfacets nrhs
//   k deg stress mode large_patches large_patches_stress
//   has_mask bvalues            bvalues: 0 no boundary values, 1 all zero, 2 one of them not zero
//   cell_nodes [3 ncells]   facet_nodes [2 nfacets]   facet_cells_off [nfacets + 1]
//   node_cells_off [nnodes + 1]   node_cells   node_facets_off [nnodes + 1]   node_facets
//   facet_type [nrhs nfacets]   node_mask [nnodes] if has_mask
//
// Every array goes to the planner as an exact-size heap block (the address sanitizer sees a read or write past it), and
// after the call the program checks that nothing but the BoundaryPlan was written: the inputs still hold what was
// read.  It also checks the tile-size rule (choose_tile_cells) on the sizes DESIGN.md quotes.
// exit status 0: the plan or the refusal was printed; 2: bad input; 3: an input was written to; 4: tile-size rule.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <vector>

#include "../dolfinx_eqlb_amd/csrc/eqlb_boundary_plan.h"

namespace
{
size_t wsym_doubles(int k, int64_t n) { return (size_t)(k * n * n + n); }

template <typename T>
std::vector<T> read(std::istream& in, size_t n)
{
  std::vector<T> v(n);
  for (size_t i = 0; i < n; ++i)
  {
    long long x;
    if (!(in >> x))
    {
      fprintf(stderr, "input ends early\n");
      exit(2);
    }
    v[i] = (T)x;
  }
  v.shrink_to_fit();
  return v;
}

template <typename T>
void print(const char* name, const std::vector<T>& v)
{
  printf("%s", name);
  for (const T& x : v)
    printf(" %lld", (long long)x);
  printf("\n");
}

int check_tile_size_rule()
{
  // tile sizes of the example in the comment of choose_tile_cells: default, EV mode of RT_3, upper limit
  const eqlb::TileSizes ts{448, 256, 489};
  auto choose_tile_cells = [&](int k, int mode, int64_t nc, int tc_fixed, int user) {
    return eqlb::choose_tile_cells(k, mode, nc, tc_fixed, user, ts);
  };
  const bool ok = choose_tile_cells(2, 0, 1000000, 0, 0) == 489    // 2 048 tiles: 4 whole rounds of 512 slots
                  && choose_tile_cells(2, 0, 1000, 0, 0) == 448    // a small mesh: the default
                  && choose_tile_cells(2, 0, 1000, 0, 100) == 100  // option "tile_cells" ...
                  && choose_tile_cells(2, 0, 1000, 0, 9999) == 489 // ... capped by the LDS
                  && choose_tile_cells(3, 1, 1000, 0, 0) == 256    // EV mode of RT_3
                  && choose_tile_cells(2, 0, 1000000, 524, 0) == 489 // fused stress launch: 8 rounds of 256 slots
                  && choose_tile_cells(2, 0, 1000, 524, 0) == 448 && choose_tile_cells(2, 0, 1000, 524, 600) == 524;
  if (!ok)
    fprintf(stderr, "choose_tile_cells: unexpected tile size\n");
  return ok ? 0 : 4;
}
} // namespace

int main(int argc, char** argv)
{
  if (argc != 2)
    return 2;
  if (const int st = check_tile_size_rule())
    return st;
  std::ifstream in(argv[1]);
  const auto dim = read<int32_t>(in, 4);
  const auto opt = read<int>(in, 6);
  const auto aux = read<int>(in, 2);
  const int32_t nnodes = dim[0], ncells = dim[1], nfacets = dim[2], nrhs = dim[3];
  const auto cell_nodes = read<int32_t>(in, 3 * (size_t)ncells);
  const auto facet_nodes = read<int32_t>(in, 2 * (size_t)nfacets);
  const auto facet_cells_off = read<int32_t>(in, (size_t)nfacets + 1);
  const auto node_cells_off = read<int32_t>(in, (size_t)nnodes + 1);
  const auto node_cells = read<int32_t>(in, (size_t)node_cells_off[nnodes]);
  const auto node_facets_off = read<int32_t>(in, (size_t)nnodes + 1);
  const auto node_facets = read<int32_t>(in, (size_t)node_facets_off[nnodes]);
  const auto facet_type = read<int8_t>(in, (size_t)nrhs * nfacets);
  const auto mask = aux[0] ? read<uint8_t>(in, (size_t)nnodes) : std::vector<uint8_t>();
  std::vector<int32_t> node_ncells(nnodes), node_nfcts(nnodes), node_nbnd(nnodes);
  for (int32_t i = 0; i < nnodes; ++i)
  {
    node_ncells[i] = node_cells_off[i + 1] - node_cells_off[i];
    node_nfcts[i] = node_facets_off[i + 1] - node_facets_off[i];
  }
  eqlb::count_node_boundary_facets(nnodes, node_facets_off.data(), node_facets.data(), facet_cells_off.data(),
                                   node_nbnd.data());
  const int nrt = opt[0] * (opt[0] + 2);
  std::vector<double> bvalues(aux[1] ? (size_t)nrhs * ncells * nrt : 0, 0.0);
  if (aux[1] == 2)
    bvalues.back() = 1.5;

  const eqlb::HostTopology topo{nnodes, ncells, nfacets, node_ncells.data(), node_nfcts.data(), node_nbnd.data(),
                                cell_nodes.data(), facet_nodes.data(), facet_cells_off.data(), node_facets_off.data(),
                                node_facets.data(), node_cells_off.data(), node_cells.data()};
  const eqlb::PlanOptions o{opt[0], opt[1], nrhs, nrt, opt[2], opt[3], opt[4], opt[5], wsym_doubles};
  const auto c_cell_nodes = cell_nodes, c_facet_nodes = facet_nodes, c_fco = facet_cells_off, c_nco = node_cells_off,
             c_nc = node_cells, c_nfo = node_facets_off, c_nf = node_facets, c_n1 = node_ncells, c_n2 = node_nfcts,
             c_n3 = node_nbnd;
  const auto c_ft = facet_type;
  const auto c_mask = mask;
  const auto c_bv = bvalues;

  eqlb::BoundaryPlan p;
  const int code = eqlb::plan_boundary(topo, o, facet_type.data(), aux[1] ? bvalues.data() : nullptr,
                                       aux[0] ? mask.data() : nullptr, p);

  if (c_cell_nodes != cell_nodes || c_facet_nodes != facet_nodes || c_fco != facet_cells_off || c_nco != node_cells_off
      || c_nc != node_cells || c_nfo != node_facets_off || c_nf != node_facets || c_n1 != node_ncells
      || c_n2 != node_nfcts || c_n3 != node_nbnd || c_ft != facet_type || c_mask != mask || c_bv != bvalues)
  {
    fprintf(stderr, "plan_boundary wrote to its inputs\n");
    return 3;
  }
  printf("code %d\n", code);
  if (code)
  {
    printf("message %s\n", p.message.c_str());
    return 0;
  }
  printf("flags %d %d %d %d %d %d %d %d\n", (int)p.inhomogeneous, (int)p.stress_flux_bcs, (int)p.stress_fused_ok,
         (int)p.tiles, (int)p.t_stress, (int)p.t_mixed, p.ws_levels, (int)p.any);
  print("node_bin", p.node_bin);
  print("node_slot", p.node_slot);
  print("node_patch", p.node_patch);
  for (int b = 0; b < eqlb::MAX_BINS; ++b)
    printf("bin %d %lld %lld %lld %lld\n", p.bins[b].P, (long long)p.bins[b].npatch, (long long)p.bins[b].slot_offset,
           (long long)p.bins[b].patch_offset, (long long)p.bins[b].nfull);
  printf("totals %lld %lld %d %lld\n", (long long)p.nslots, (long long)p.npatch_total, (int)p.l_maxcells,
         (long long)p.t_rest);
  print("large_nodes", p.large_nodes);
  print("l_off", p.l_off);
  print("l_cells", p.l_cells);
  print("l_wsym_off", p.l_wsym_off);
  print("ws", p.ws);
  print("group", p.group);
  print("level", p.level);
  print("tile_bin", p.tile_bin);
  print("rest_cells", p.rest_cells);
  print("l_rest_cells", p.l_rest_cells);
  return 0;
}
