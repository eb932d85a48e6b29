"""Name registries: drop-in SearchFactory (utils/planner/search_factory.py:13-51), ControlFactory
(utils/planner/control_factory.py:13-27) and CurveFactory (utils/planner/curve_factory.py:9-29) for the
planners and curves this package accelerates.  Names of
reference planners outside the accelerated hot path raise NotImplementedError (not silently
substituted)."""
from __future__ import annotations

# "aco" has a class (evolutionary_search.ACO, csrc/aco.hip) but, like "jps" and "rrt_connect", its factory name
# keeps raising: construct the class
_SEARCH_OUT_OF_SCOPE = {"jps", "voronoi", "s_theta_star", "anya", "rrt_connect", "aco"}
# PID / APF / RPP exist as classes (local_planner.PID, APF, RPP); like "jps", their factory names keep
# raising
_CONTROL_OUT_OF_SCOPE = {"pid", "apf", "rpp"}


class SearchFactory(object):
    def __call__(self, planner_name, **config):
        from . import graph_search

        table = {"a_star": "AStar", "dijkstra": "Dijkstra", "gbfs": "GBFS", "d_star": "DStar", "rrt": "RRT",
                 "rrt_star": "RRTStar", "informed_rrt": "InformedRRT", "theta_star": "ThetaStar", "lazy_theta_star": "LazyThetaStar",
                 "lpa_star": "LPAStar", "d_star_lite": "DStarLite"}
        if planner_name in table:
            mod = graph_search if planner_name in ("a_star", "dijkstra", "gbfs", "d_star", "theta_star", "lazy_theta_star", "lpa_star", "d_star_lite") else __import__(
                __package__ + ".sample_search", fromlist=["x"])
            cls = getattr(mod, table[planner_name], None)
            if cls is None:
                raise NotImplementedError(f"{planner_name} is not implemented yet in python_motion_planning_amd")
            return cls(**config)
        if planner_name == "pso":
            from . import evolutionary_search

            return evolutionary_search.PSO(**config)
        if planner_name in _SEARCH_OUT_OF_SCOPE:
            raise NotImplementedError(f"{planner_name} is outside the accelerated hot path of python_motion_planning_amd")
        raise ValueError("The `planner_name` must be set correctly.")


class ControlFactory(object):
    def __call__(self, planner_name, **config):
        from . import local_planner

        table = {"dwa": "DWA", "lqr": "LQR", "mpc": "MPC"}
        if planner_name in table:
            cls = getattr(local_planner, table[planner_name], None)
            if cls is None:
                raise NotImplementedError(f"{planner_name} is not implemented yet in python_motion_planning_amd")
            return cls(**config)
        if planner_name in _CONTROL_OUT_OF_SCOPE:
            raise NotImplementedError(f"{planner_name} is not a ControlFactory name of python_motion_planning_amd; "
                                      f"construct python_motion_planning_amd.{planner_name.upper()} directly")
        raise ValueError("The `planner_name` must be set correctly.")


# the reference's curve names (utils/planner/curve_factory.py:14-27) the factory refuses: three with no kernel
# here, and "reeds_shepp", "polynomial" and "bezier", which have one (curve.ReedsShepp, csrc/reeds_shepp.hip;
# curve.Polynomial and curve.Bezier, csrc/polycurve.hip) but keep their refusal as "jps", "rrt_connect" and
# "pid" do in their factories: construct the class
_CURVE_OUT_OF_SCOPE = {"bezier", "polynomial", "reeds_shepp", "cubic_spline", "bspline", "fem_pos_smoother"}


class CurveFactory(object):
    def __call__(self, curve_name, **config):
        from . import curve

        if curve_name == "dubins":
            return curve.Dubins(**config)
        if curve_name in _CURVE_OUT_OF_SCOPE:
            raise NotImplementedError(f"{curve_name} is outside the accelerated hot path of python_motion_planning_amd")
        raise ValueError("The `curve_name` must be set correctly.")
