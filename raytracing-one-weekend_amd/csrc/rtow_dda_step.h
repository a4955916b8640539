// rtow_dda_step.h — one cell crossing of the uniform-grid walk (rtow_trace_grid.h), in two forms: the 3D-DDA, and the
// two-axis form for a grid whose y axis is a single layer of cells (grid_header() of rtow_grid.h collapses a thin axis:
// the cover scenes are 35 x 1 x 35).  Plain C++ without includes, so that the kernels (inside their namespace) and a host
// test program (tests/tools/flat_dda_check.cpp) compile the very same functions.
//
// Contract of both: the lane stands in cell `idx`; the step leaves it through the nearest cell wall — x before y before z
// when parameters are equal — and returns whether the walk goes on: the cell behind that wall exists (integer counters,
// so a walk ends after at most nx + ny + nz steps whatever the floats do) and starts no later than `tmax`.  `t_entry`
// becomes the ray parameter of the wall.  After a step that returns false the state is dead: nothing reads it again.
//
// With ny == 1 the y wall of EVERY cell is the slab's exit plane: tmy never changes and remy is 0, so a step through y
// always ends the walk.  The two-axis form keeps that one parameter (`ty_exit`) and drops the y cell, increment, stride
// and counter.  It takes the same decisions from the same comparisons: an x step wins tmx == ty_exit, the exit wins
// ty_exit == tmz; and since a y step ends the walk, "not x" may update the z state unconditionally (dead when y won).
#pragma once

#if defined(__HIPCC__) || defined(__CUDACC__)
#define RTOW_DDA_FN __host__ __device__ __forceinline__
#else
#define RTOW_DDA_FN inline
#endif

struct DdaWalk3 {
  float tmx, tmy, tmz;  // ray parameter of the next wall per axis
  float tdx, tdy, tdz;  // parameter per cell
  int remx, remy, remz;  // cells left in the direction of travel
  int incx, incy, incz;  // cell index stride, signed
  int idx;
};

struct DdaWalk2 {
  float tmx, tmz;
  float tdx, tdz;
  float ty_exit;  // where the ray leaves the slab through y: the generic walk's tmy, constant for the ray
  int remx, remz;
  int incx, incz;
  int idx;  // c2 * nx + c0
};

template <bool FLAT>
struct DdaWalkOf {
  using type = DdaWalk3;
};
template <>
struct DdaWalkOf<true> {
  using type = DdaWalk2;
};

// (Both read the state into values first: a select between two MEMBERS becomes a load through a selected address, and
// the state then lives in scratch memory instead of registers.)
RTOW_DDA_FN bool dda_step(DdaWalk3 &w, float tmax, float &t_entry) {
  const float tmx = w.tmx, tmy = w.tmy, tmz = w.tmz, tdx = w.tdx, tdy = w.tdy, tdz = w.tdz;
  const int remx = w.remx, remy = w.remy, remz = w.remz, incx = w.incx, incy = w.incy, incz = w.incz;
  // leave through the nearest cell wall (x before y before z when equal): one v_min3 and two equality tests
  const float tnext = __builtin_fminf(__builtin_fminf(tmx, tmy), tmz);
  const bool sx = tmx == tnext;
  const bool sy = !sx && tmy == tnext;
  const int rem = sx ? remx : (sy ? remy : remz);
  const bool walking = rem > 0 && !(tnext > tmax);
  t_entry = tnext;
  w.idx += sx ? incx : (sy ? incy : incz);
  w.tmx = tmx + (sx ? tdx : 0.0f);
  w.tmy = tmy + (sy ? tdy : 0.0f);
  w.tmz = tmz + ((!sx && !sy) ? tdz : 0.0f);
  w.remx = remx - (sx ? 1 : 0);
  w.remy = remy - (sy ? 1 : 0);
  w.remz = remz - ((!sx && !sy) ? 1 : 0);
  return walking;
}

RTOW_DDA_FN bool dda_step(DdaWalk2 &w, float tmax, float &t_entry) {
  const float tmx = w.tmx, tmz = w.tmz, tdx = w.tdx, tdz = w.tdz, ty_exit = w.ty_exit;
  const int remx = w.remx, remz = w.remz, incx = w.incx, incz = w.incz;
  const float tnext = __builtin_fminf(__builtin_fminf(tmx, ty_exit), tmz);
  const bool sx = tmx == tnext;
  const bool sy = !sx && ty_exit == tnext;  // out of the slab: the generic walk's remy == 0
  const int rem = sx ? remx : remz;
  const bool walking = rem > 0 && !sy && !(tnext > tmax);
  t_entry = tnext;
  // selects, no branches; "not x" stands for z (when y won, the walk is over and the state dead)
  w.idx += sx ? incx : incz;
  w.tmx = tmx + (sx ? tdx : 0.0f);
  w.tmz = tmz + (sx ? 0.0f : tdz);
  w.remx = remx - (sx ? 1 : 0);
  w.remz = remz - (sx ? 0 : 1);
  return walking;
}
