// Inputs of the test case list for tests/native/traj_limits_sanitize_main.cpp: durations, coefficients (6N x 3 column-major) and the
// reference extrema of tests/golden/traj_limits.npz, written by tests/golden/make_golden_limits.py's numbers as exact hexadecimal
// floating-point literals.  Data only.
struct GoldenCase { const char *name; int N; const double *T, *C, *value, *time; };
static const double n1_mid_T[] = {0x1.0000000000000p+0};
static const double n1_mid_C[] = {0x1.fd80000000000p+6, 0x1.8000000000000p+0, 0x1.0000000000000p+0, 0x1.0000000000000p-1, -0x1.e000000000000p+1, 0x1.0000000000000p+1, 0x1.00dbbbbbbbbbcp+7, -0x1.0000000000000p+0, -0x1.8000000000000p-1, -0x1.5555555555555p-2, 0x1.5000000000000p+1, -0x1.6666666666666p+0, 0x1.ff0cccccccccdp+6, 0x1.0000000000000p-1, 0x1.0000000000000p-1, 0x1.0000000000000p-2, -0x1.a000000000000p+0, 0x1.b333333333333p-1};
static const double n1_mid_value[] = {0x1.3704e89979b3fp+1, 0x1.5b3f551c380e2p+2, 0x1.06b094a26c57fp+2, 0x1.19051eaf053b8p-1, 0x1.b8e3112ac11cdp+2, 0x1.6aeec73590017p+2};
static const double n1_mid_time[] = {0x1.335705d516150p-2, 0x1.6ed4a24f275f4p-1, 0x1.0000000000000p+0, 0x1.73774f807c808p-1, 0x1.5dec065f621c7p-5, 0x1.d15f5487c4392p-1};
static const double n1_tilted_T[] = {0x1.0000000000000p+0};
static const double n1_tilted_C[] = {0x1.ff263f8cc6b6ap+6, 0x0.0p+0, 0x1.5f8ab4a96ee58p+0, 0x1.1111111111111p-3, -0x1.2141a118acc5bp+1, 0x1.2db6a5026d327p+0, 0x1.ff529b5ea5807p+6, 0x0.0p+0, 0x1.28197eb346612p+0, -0x1.5555555555555p-4, -0x1.9c263e0ce991bp+0, 0x1.c028cab8709b6p-1, 0x1.022f9f9cf9fefp+7, 0x0.0p+0, -0x1.d36b6936bade9p+2, 0x1.9999999999999p-5, 0x1.5c2a2882a5c08p+3, -0x1.7404024043935p+2};
static const double n1_tilted_value[] = {0x1.f3b520bc0cec7p+1, 0x1.e1561540f146dp+3, 0x1.1e9a025ebd21dp+4, 0x1.400808f29be40p+1, 0x1.8040052b6847dp+3, 0x1.72fbcefb96a8ap+0};
static const double n1_tilted_time[] = {0x1.af7bab513ba54p-2, 0x0.0p+0, 0x1.ee0efc050fc0bp-3, 0x1.5fe4a6ff78b15p-8, 0x1.8339c5c6ea1e5p-1, 0x1.e653c507e0662p-3};
static const double n1_omg_T[] = {0x1.0000000000000p+0};
static const double n1_omg_C[] = {0x1.ff7ae147ae148p+6, 0x1.999999999999ap-2, 0x1.0000000000000p+0, -0x1.6666666666667p+1, 0x1.2666666666666p+1, -0x1.47ae147ae147ap-1, 0x1.fff6e1d741984p+6, 0x1.999999999999ap-3, -0x1.8000000000000p-1, 0x1.1999999999999p+0, -0x1.7333333333332p-1, 0x1.70a3d70a3d706p-3, 0x1.ffc34e626eeefp+6, -0x1.999999999999ap-4, 0x1.0000000000000p-1, 0x1.5555555555555p-2, -0x1.2666666666666p+0, 0x1.147ae147ae146p-1};
static const double n1_omg_value[] = {0x1.179ce5d919053p-1, 0x1.58a68a4a8d9f3p+1, 0x1.9910eb2394749p+0, 0x1.d8a472ad7d8a3p-3, 0x1.b07454a8a1d20p+2, 0x1.63d5604e866c9p+2};
static const double n1_omg_time[] = {0x1.59c943012ee85p-3, 0x0.0p+0, 0x0.0p+0, 0x0.0p+0, 0x0.0p+0, 0x1.908094535e920p-1};
static const double n2_junction_T[] = {0x1.0000000000000p+0, 0x1.0000000000000p+0};
static const double n2_junction_C[] = {0x1.ffe0000000000p+6, -0x1.4000000000000p-2, 0x1.4000000000000p-1, -0x1.8800000000000p+1, 0x1.0400000000000p+2, -0x1.4800000000000p+0, 0x1.0000000000000p+7, 0x1.9800000000000p+0, -0x1.8000000000000p+1, 0x1.8000000000000p-2, 0x1.2c00000000000p+1, -0x1.3800000000000p+0, 0x1.0020000000000p+7, 0x0.0p+0, 0x0.0p+0, 0x1.a000000000000p+0, -0x1.4000000000000p+1, 0x1.a000000000000p-1, 0x1.0000000000000p+7, -0x1.1000000000000p+0, 0x1.0000000000000p+1, -0x1.0000000000000p-2, -0x1.9000000000000p+0, 0x1.a000000000000p-1, 0x1.ffa0000000000p+6, 0x1.4000000000000p-2, -0x1.4000000000000p-1, -0x1.8000000000000p-3, 0x1.e000000000000p-1, -0x1.6000000000000p-2, 0x1.0000000000000p+7, 0x1.1000000000000p-1, -0x1.0000000000000p+0, 0x1.0000000000000p-3, 0x1.9000000000000p-1, -0x1.a000000000000p-2};
static const double n2_junction_value[] = {0x1.fcdd8b27ec33ep+0, 0x1.deeea11683f49p+2, 0x1.2b6ed06e83bcep+1, 0x1.6f9abdc85c820p-1, 0x1.12b75005addedp+3, 0x1.4ee4efbf58ad0p+2};
static const double n2_junction_time[] = {0x1.0000000000000p+0, 0x1.0000000000000p+0, 0x0.0p+0, 0x1.0000000000000p+0, 0x1.0000000000000p+0, 0x1.ffbc93f0b6c29p-5};
static const double n1_monotone_T[] = {0x1.8000000000000p+0};
static const double n1_monotone_C[] = {0x1.0000000000000p+7, 0x1.3333333333333p-2, 0x1.cccccccccccccp-2, 0x1.3333333333333p-3, 0x0.0p+0, 0x0.0p+0, 0x1.0000000000000p+7, 0x0.0p+0, 0x0.0p+0, 0x0.0p+0, 0x0.0p+0, 0x0.0p+0, 0x1.0000000000000p+7, 0x1.999999999999ap-2, 0x1.3333333333334p-1, 0x1.999999999999ap-3, 0x0.0p+0, 0x0.0p+0};
static const double n1_monotone_value[] = {0x1.1c00000000000p+2, 0x1.e000000000000p+1, 0x1.555b85bc8018fp-4, 0x1.97d4ed325208ep-3, 0x1.0aff1e4027860p+3, 0x1.b199969be452ap+2};
static const double n1_monotone_time[] = {0x1.8000000000000p+0, 0x1.8000000000000p+0, 0x0.0p+0, 0x1.8000000000000p+0, 0x1.8000000000000p+0, 0x0.0p+0};
static const GoldenCase GOLDEN_CASES[] = {
    {"n1_mid", 1, n1_mid_T, n1_mid_C, n1_mid_value, n1_mid_time},
    {"n1_tilted", 1, n1_tilted_T, n1_tilted_C, n1_tilted_value, n1_tilted_time},
    {"n1_omg", 1, n1_omg_T, n1_omg_C, n1_omg_value, n1_omg_time},
    {"n2_junction", 2, n2_junction_T, n2_junction_C, n2_junction_value, n2_junction_time},
    {"n1_monotone", 1, n1_monotone_T, n1_monotone_C, n1_monotone_value, n1_monotone_time},
};
