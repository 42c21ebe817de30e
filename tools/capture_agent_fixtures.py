#!/usr/bin/env python3
"""Captures the `agent_*` fixtures of the reference's three later env-reading heuristics (ChargeAsLateAsPossibleToDesiredCapacity,
RoundRobin_GF, RoundRobin_GF_off_allowed) with oracle/capture_golden.run_case: the reference's agent and the same-named agent of
ev2gym_amd.baselines.heuristics drive one reference env in lockstep, equal actions are asserted at every step, the trajectory is recorded.

Needs a checkout of the upstream reference where oracle/ref_import.py expects it.  Writes tests/golden/<name>.npz (EV2G_GOLDEN_OUT
redirects, as for oracle/capture_golden.py); names given on the command line select cases.

    python tools/capture_agent_fixtures.py [name ...]
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))   # capture_golden imports its siblings by their bare names
sys.path.insert(1, ROOT)

import capture_golden as cg  # noqa: E402

PPL = ("V2G_profit_max_loads", "ProfitMax_TrPenalty_UserIncentives")
PST = ("PublicPST", "SquaredTrackingErrorReward")


def cases():
    base = "ev2gym/example_config_files/"
    ppl, pst = base + "V2GProfitPlusLoads.yaml", base + "PublicPST.yaml"
    des80 = cg._yaml_variant(ppl, {"ev": {"desired_capacity": 0.8}}, "v2gppl_des80")   # the afapdes fixture's variant
    setpoints = cg._yaml_variant(ppl, {"power_setpoint_enabled": True}, "v2gppl_setpoints")   # one port per charger, as shipped
    return [("agent_calapdes_v2gppl_des80_s67", des80, *PPL, 67, "agent:ChargeAsLateAsPossibleToDesiredCapacity", None),
            ("agent_rrgf_pst_s68", pst, *PST, 68, "agent:RoundRobin_GF", None),
            ("agent_rrgfoff_pst_s69", pst, *PST, 69, "agent:RoundRobin_GF_off_allowed", None),
            ("agent_rrgf_v2gppl_setpoints_s70", setpoints, *PPL, 70, "agent:RoundRobin_GF", None)]


def main():
    cg.import_reference()
    only = set(sys.argv[1:])
    for c in cases():
        if not only or c[0] in only:
            cg.run_case(*c)


if __name__ == "__main__":
    main()
