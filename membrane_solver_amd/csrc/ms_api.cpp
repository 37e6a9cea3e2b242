// Host side of libmembrane_hip.so: context management, HBM residency, the
// device-resident minimizer step, and the extern "C" ABI of
// include/membrane_hip.h.  Arithmetic lives in ms_kernels.hip.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <algorithm>
#include <cstring>
#include <ctime>
#include <map>
#include <string>
#include <new>

#include <dlfcn.h>

#include "ms_internal.h"
#include "ms_slot_writers.h"
#include "ms_table_blob.h"
#include "ms_test_hooks.h"

static void shard_comm_destroy(void* comm);  // (RCCL binding further down)

using namespace ms;

namespace {
std::string g_last_error;  // for failures that have no context yet
}

#include "ms_api_ctx.inc"  // the context: everything a ms_ctx holds
#include "ms_api_phases.inc"  // pass launchers, folds, mailboxes, the energy / gradient / direction phases
#include "ms_api_tables.inc"  // what the ring and rim setters share: the plane check and its axes, a ring's external rows
#include "ms_api_edge.inc"  // line_tension and edge_length_penalty: the edge / vertex tables, each term's two launches behind the energy and the gradient pass
#include "ms_api_rim.inc"  // tilt_rim_source_in/out: the rim tables, the frame / coefficient / apply launches next to the disk-target pass
#include "ms_api_rimmatch.inc"  // rim_slope_match_out: the three rings' rows and frame, the geometry / apply launches
#include "ms_api_thetab.inc"  // tilt_thetaB_contact_in: the ring's rows and frame, theta_B, the geometry / apply launches, the scalar update
#include "ms_api_couple.inc"  // tilt_coupling: its setter and getters, its pass
#include "ms_api_splay.inc"  // tilt_splay_twist_in: its setter and getters, its pass
#include "ms_api_addons.inc"  // the leaflet add-on passes above in the slot-writer table's order, each with its cell mode
#include "ms_api_pins.inc"  // pin_to_plane / pin_to_circle: tables, the enforcement program, the project lane
#include "ms_api_area_con.inc"  // body_area / global_area: the setter, the area row's part in the gradient projection, the enforcer loop
#include "ms_api_enforce.inc"  // fixed_plane / perimeter: the setters, perimeter's table builder, the two enforcer launches
#include "ms_api_context.inc"  // create / destroy, setters and getters, curvature fields
#include "ms_api_tilt.inc"  // tilt-module evaluation, the relaxations (host-driven, device program, fused), leaflet fields
#include "ms_api_thetab_bnd.inc"  // tilt_thetaB_boundary_in: the constraint's ring and row -> facet CSR, the geometry / apply launches of the relaxation, the cadence
#include "ms_api_step.inc"  // energy / gradient entry points, line-search rounds, ms_step, volume projection, the resident step, ms_minimize
#include "ms_api_shard.inc"  // phase API, boundary exchange, the sharded drivers (RCCL, peer-to-peer), ms_shard_step
#include "ms_api_misc.inc"  // state rebinding, statistics, profiling, the tiling planner, the kernel-provider seam
