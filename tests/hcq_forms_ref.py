"""The 8-multiplication Hamilton product of csrc/hcq_forms.h restated for the host-side bounds (no GPU): P_m = F_m(a) G_m(b),
2 c_q = sum_m R2[q][m] P_m.  F and G as (component, component): only which two components a form sums matters to a bound."""
HCQ_F = ((3, 1), (0, 2), (0, 2), (3, 1), (3, 2), (1, 0), (0, 1), (3, 2))
HCQ_G = ((1, 2), (0, 3), (0, 3), (1, 2), (2, 3), (1, 0), (2, 3), (1, 0))
HCQ_R2 = ((-1, 1, 1, 1, 2, 0, 0, 0), (-1, -1, -1, 1, 0, 2, 0, 0), (1, -1, 1, 1, 0, 0, 2, 0), (1, 1, -1, 1, 0, 0, 0, -2))
