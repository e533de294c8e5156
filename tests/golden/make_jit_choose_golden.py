"""Writes the fixtures of tests/test_host_jit_choose.py: jit_choices.txt.gz, jit_candidates.txt.gz, jit_wisdom_rows.json, jit_pin_rows.json.

    python tests/golden/make_jit_choose_golden.py        (after __graft_entry__.build())

They record what the plan-time chooser answered when csrc/jit.cpp still held it in one piece, through tests/jit_choose_driver.cpp linked
with that library's objects -- the reference for every later change to the chooser, so they are NOT to be refreshed from a chooser that
answers something else: then the chooser is wrong.  The one exception is written by hand: the rows of jit_pin_rows.json with a "rule"
entry pin a factorization that needs more than 16 points per thread in some stage; they expect the answer without the pin."""
import json
import os
import sys
import tempfile

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import jit_choose_lib as J      # noqa: E402
import plan_driver              # noqa: E402

K1280 = "fused v1 gfx950t 1280 4 f"       # (gfx950t: the device part of the keys below)

# (name, text of wisdom.txt, request).  640x480 u2: rows of 1280, the chooser picks 16*16*5, the built-in table 256:8,10,16
WISDOM = [
    ("valid_differs_from_pick", K1280 + " = 320:8,4,8,5\n", "choose 640 480 4 1 0 1 gfx950t"),
    ("valid_but_wisdom_not_asked", K1280 + " = 320:8,4,8,5\n", "choose 640 480 4 1 0 0 gfx950t"),
    ("other_device_key", "fused v1 gfx942 1280 4 f = 320:8,4,8,5\n", "choose 640 480 4 1 0 1 gfx950t"),
    ("equal_to_pick", "fused v1 gfx950t 2000 4 f = 256:8,5,5,10\n", "choose 1000 1000 4 1 0 1 gfx950t"),
    ("equal_to_pick_as_stored", "fused v1 gfx950t 2000 4 f = 256:8, 5, 5, 10\n", "choose 1000 1000 4 1 0 1 gfx950t"),
    ("pow2_keeps_the_default", K1280 + " = pow2\n", "choose 640 480 4 1 0 1 gfx950t"),
    ("mr16_keeps_the_default", K1280 + " = mr16\n", "choose 640 480 4 1 0 1 gfx950t"),
    ("wrong_product", K1280 + " = 256:8,10,8\n", "choose 640 480 4 1 0 1 gfx950t"),
    ("non_radix_factor", K1280 + " = 256:20,8,8\n", "choose 640 480 4 1 0 1 gfx950t"),
    ("threads_not_a_multiple_of_64", K1280 + " = 200:8,10,16\n", "choose 640 480 4 1 0 1 gfx950t"),
    ("threads_below_n_over_r0", K1280 + " = 128:8,10,16\n", "choose 640 480 4 1 0 1 gfx950t"),
    ("threads_above_1024", K1280 + " = 1088:8,10,16\n", "choose 640 480 4 1 0 1 gfx950t"),
    ("over_16_points_16_12_16", "fused v1 gfx950t 3072 4 f = 192:16,12,16\n", "choose 1536 480 4 1 0 1 gfx950t"),
    ("over_16_points_16_3_16_8", "fused v1 gfx950t 6144 4 f = 384:16,3,16,8\n", "choose 3072 480 4 1 0 1 gfx950t"),
    ("within_16_points_16_3_16", "fused v1 gfx950t 768 4 f = 64:16,3,16\n", "choose 384 480 4 1 0 1 gfx950t"),
    ("first_radix_not_a_multiple_of_the_factor", "fused v1 gfx950t 1920 6 f = 256:8,15,16\n", "choose 640 480 6 1 0 1 gfx950t"),
    ("quarter_factor_key", "fused v1 gfx950t 800 5/2 f = 128:10,8,10\n", "choose 640 480 5 2 0 1 gfx950t"),
    ("half_precision_key", "fused v1 gfx950t 1280 4 h = 320:8,4,8,5\n", "choose 640 480 4 1 1 1 gfx950t"),
    ("half_precision_key_other_precision", "fused v1 gfx950t 1280 4 h = 320:8,4,8,5\n", "choose 640 480 4 1 0 1 gfx950t"),
    ("two_lines_last_wins", K1280 + " = 320:8,4,8,5\n" + K1280 + " = 256:16,8,10\n", "choose 640 480 4 1 0 1 gfx950t"),
    ("two_lines_last_invalid", K1280 + " = 320:8,4,8,5\n" + K1280 + " = 256:8,10,8\n", "choose 640 480 4 1 0 1 gfx950t"),
    ("malformed_word", K1280 + " = garbage\n", "choose 640 480 4 1 0 1 gfx950t"),
    ("malformed_no_radices", K1280 + " = 256:\n", "choose 640 480 4 1 0 1 gfx950t"),
    ("malformed_no_threads", K1280 + " = :8,10,16\n", "choose 640 480 4 1 0 1 gfx950t"),
    ("malformed_no_colon", K1280 + " = 8,10,16\n", "choose 640 480 4 1 0 1 gfx950t"),
    ("malformed_empty_factor", K1280 + " = 256:8,,10,16\n", "choose 640 480 4 1 0 1 gfx950t"),
    ("malformed_one_factor", K1280 + " = 1024:1280\n", "choose 640 480 4 1 0 1 gfx950t"),
    ("malformed_no_separator", K1280 + "=320:8,4,8,5\nnot a line\n\n", "choose 640 480 4 1 0 1 gfx950t"),
]

# (name, FFTUP_EXPERIMENT, request, None): the build with the test knobs.  The rows written by hand (see above) have, in place of
# None, the experiment whose answer they expect: the same without the pin, or with a pin that was ignored all along
PINS = [
    ("row_valid", "jit_row=5,8,16", "choose 640 480 4 1 0 1 -", None),
    ("row_wrong_product", "jit_row=5,8,8", "choose 640 480 4 1 0 1 -", None),
    ("row_non_radix", "jit_row=20,4,8", "choose 640 480 4 1 0 1 -", None),
    ("row_four_factors_without_nstage", "jit_row=4,4,5,8", "choose 640 480 4 1 0 1 -", None),
    ("row_nstage", "jit_row_nstage", "choose 640 480 4 1 0 1 -", None),
    ("row_nstage_valid", "jit_row_nstage;jit_row=4,4,5,8", "choose 640 480 4 1 0 1 -", None),
    ("row_nstage_three_factors", "jit_row_nstage;jit_row=5,8,16", "choose 640 480 4 1 0 1 -", None),
    ("row_nstage_wrong_product", "jit_row_nstage;jit_row=4,4,5,4", "choose 640 480 4 1 0 1 -", None),
    ("row_nstage_non_radix", "jit_row_nstage;jit_row=4,4,40", "choose 640 480 4 1 0 1 -", None),
    ("row_nstage_one_factor", "jit_row_nstage;jit_row=640", "choose 640 480 4 1 0 1 -", None),
    ("row_nstage_too_many_threads", "jit_row_nstage;jit_row=2,15,16,2,4", "choose 3840 480 4 1 0 1 -", None),
    ("row_nstage_over_16_points", "jit_row_nstage;jit_row=16,12,16", "choose 3072 480 4 1 0 1 -", "jit_row_nstage"),
    # (three stages run on the threads of the stage with the smallest radix, one butterfly each: a small middle radix is fine)
    ("row_small_middle_radix_16_5_16", "jit_row=16,5,16", "choose 1280 480 4 1 0 1 -", None),
    ("row_small_middle_radix_16_3_16", "jit_row=16,3,16", "choose 768 480 4 1 0 1 -", None),
    ("row_small_middle_radix_16_7_16", "jit_row=16,7,16", "choose 1792 480 4 1 0 1 -", None),
    ("row_threads_prefix_is_ignored", "jit_row=64:5,8,16", "choose 640 480 4 1 0 1 -", None),
    ("col_valid", "jit_col=2,15,16", "choose 640 480 4 1 0 1 -", None),
    ("col_wrong_product", "jit_col=2,15,8", "choose 640 480 4 1 0 1 -", None),
    ("col_non_radix", "jit_col=6,5,16", "choose 640 480 4 1 0 1 -", None),
    ("col_small_middle_radix_16_3_16", "jit_col=16,3,16", "choose 640 768 4 1 0 1 -", None),
    ("col_small_middle_radix_15_2_16", "jit_col=15,2,16", "choose 640 480 4 1 0 1 -", None),
    ("col_nstage", "jit_col_nstage", "choose 640 480 4 1 0 1 -", None),
    ("col_nstage_valid", "jit_col_nstage;jit_col=4,2,4,15", "choose 640 480 4 1 0 1 -", None),
    ("col_nstage_two_columns", "jit_col_nstage;jit_col=5,12,4,8", "choose 640 1920 4 1 0 1 -", None),
    ("col_nstage_too_many_threads", "jit_col_nstage;jit_col=2,4,15,16", "choose 640 1920 4 1 0 1 -", None),
    ("col_nstage_over_16_points", "jit_col_nstage;jit_col=16,12,16", "choose 640 3072 4 1 0 1 -", "jit_col_nstage"),
    ("col_u3_valid", "jit_col=4,2,4,15", "choose 640 480 6 1 0 1 -", None),
    ("col_half_integer_valid", "jit_col=4,2,4,15", "choose 640 480 3 1 0 1 -", None),
    ("coli_valid", "jit_coli=8,9,10", "choose 640 480 3 1 0 1 -", None),
    ("coli_wrong_product", "jit_coli=8,9,5", "choose 640 480 3 1 0 1 -", None),
    ("coli_non_radix", "jit_coli=8,90", "choose 640 480 3 1 0 1 -", None),
    ("col_and_coli", "jit_col=16,2,15;jit_coli=9,5,16", "choose 640 480 3 1 0 1 -", None),
    ("fused_valid", "jit_fused=320:8,4,8,5", "choose 640 480 4 1 0 1 -", None),
    ("fused_valid_more_threads", "jit_fused=512:8,10,16", "choose 640 480 4 1 0 1 -", None),
    ("fused_without_threads", "jit_fused=8,10,16", "choose 640 480 4 1 0 1 -", None),
    ("fused_wrong_product", "jit_fused=256:8,10,8", "choose 640 480 4 1 0 1 -", None),
    ("fused_non_radix", "jit_fused=256:20,8,8", "choose 640 480 4 1 0 1 -", None),
    ("fused_threads_not_a_multiple_of_64", "jit_fused=200:8,10,16", "choose 640 480 4 1 0 1 -", None),
    ("fused_threads_below_n_over_r0", "jit_fused=128:8,10,16", "choose 640 480 4 1 0 1 -", None),
    ("fused_threads_above_1024", "jit_fused=1088:8,10,16", "choose 640 480 4 1 0 1 -", None),
    ("fused_one_factor", "jit_fused=1024:1280", "choose 640 480 4 1 0 1 -", None),
    ("fused_first_radix_not_a_multiple_of_the_factor", "jit_fused=256:8,15,16", "choose 640 480 6 1 0 1 -", None),
    ("fused_pin_on_a_power_of_two", "jit_fused=256:8,16,16", "choose 1024 480 4 1 0 1 -", None),
    # (rows of 2880 at u1.5: neither 16*16*R nor a built-in wisdom entry, so an ignored pin leaves the answer without one)
    ("fused_over_16_points", "jit_fused=192:15,12,16", "choose 1920 480 3 1 0 1 -", "jit_fused=192:15,12,8"),
    ("fused_opt", "jit_fused_opt=1,0", "choose 1000 1000 4 1 0 1 -", None),
    ("fused_opt_zero_waves", "jit_fused_opt=0,1", "choose 1000 1000 4 1 0 1 -", None),
    ("fused_opt_malformed", "jit_fused_opt=2", "choose 1000 1000 4 1 0 1 -", None),
    ("fused_opt_on_mr16", "jit_fused_opt=1,0", "choose 896 504 4 1 0 1 -", None),
    ("no_builtin_wisdom", "jit_no_builtin_wisdom", "choose 640 480 4 1 0 1 -", None),
    ("no_builtin_wisdom_value_ignored", "jit_no_builtin_wisdom=0", "choose 640 480 4 1 0 1 -", None),
    ("unknown_key", "jit_nothing=1;;=", "choose 640 480 4 1 0 1 -", None),
]


def main():
    with tempfile.TemporaryDirectory() as d:
        exe, knobs = plan_driver.build(d, "jit_choose_driver"), plan_driver.build(d, "jit_choose_driver", knobs=True)
        empty = os.path.join(d, "empty")
        rq = J.choice_requests()
        J.write_choices(os.path.join(J.GOLDEN, "jit_choices.txt.gz"), rq, J.run(exe, rq, empty))
        rq = J.candidate_requests()
        J.write_text(os.path.join(J.GOLDEN, "jit_candidates.txt.gz"), "".join("%s = %s\n" % (q, a) for q, a in zip(rq, J.run(exe, rq, empty))))
        rows = []
        for i, (name, text, request) in enumerate(WISDOM):
            cache = os.path.join(d, "w%d" % i)
            os.makedirs(cache)
            with open(os.path.join(cache, "wisdom.txt"), "w") as f:
                f.write(text)
            rows.append({"name": name, "wisdom": text, "request": request, "expect": J.run(exe, [request], cache)[0]})
        with open(os.path.join(J.GOLDEN, "jit_wisdom_rows.json"), "w") as f:
            json.dump({"rows": rows}, f, indent=1)
        rows = []
        for (name, experiment, request, instead) in PINS:
            row = {"name": name, "experiment": experiment, "request": request, "expect": J.run(knobs, [request], empty, instead or experiment)[0]}
            if instead:
                row["rule"] = "at most 16 points per thread holds for pins too: ignored, the answer is that of " + instead
                assert name != "fused_over_16_points" or row["expect"] == J.run(knobs, [request], empty)[0]
            rows.append(row)
        with open(os.path.join(J.GOLDEN, "jit_pin_rows.json"), "w") as f:
            json.dump({"rows": rows}, f, indent=1)


if __name__ == "__main__":
    main()
