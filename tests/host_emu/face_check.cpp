// tests/host_emu/face_check.cpp -- TEST INFRASTRUCTURE ONLY (tests/test_face_records_cpu.py builds and runs it).
// The FACE records k_cells makes for cells on the grid's 0-faces (make_face_entry from the pattern offset, the pattern-info and
// pattern-order tables and the owned slots) against what the generic plan of the same cell makes (plan_cell, make_entry), for
// every sign index and every combination of face flags; and the owner of every foreign edge (face_owner) against owner_of.
#include <cstdio>
#include <cstdlib>

#include "../../mc33_c_library_amd/csrc/mc33_cell.h"
#include "../../mc33_c_library_amd/csrc/mc33_lut_data.h"
#include "../../mc33_c_library_amd/csrc/mc33_rules_data.h"

using namespace mc33;

int main(int argc, char **argv) {
	const uint32_t per = argc > 1 ? (uint32_t)atoi(argv[1]) : 20;
	Tables tab{mc33_lut, mc33_rule_words, &mc33_rule_index[0][0]};
	constexpr uint32_t lut_n = sizeof mc33_lut / sizeof mc33_lut[0];
	static uint32_t info[lut_n];
	static uint64_t order[lut_n];
	build_pattern_info(mc33_lut, lut_n, info);
	build_pattern_order(mc33_lut, lut_n, order);
	Params P{};
	P.nx = P.ny = P.nz = 64;
	GridView<float> G{nullptr, 0, 0, 0};
	uint64_t st = 0x9E3779B97F4A7C15ull;
	auto rnd = [&]() { st ^= st << 13; st ^= st >> 7; st ^= st << 17; return (uint32_t)(st >> 32); };
	long checked = 0;
	for (uint32_t flags = 0; flags < 8; flags++) {
		const uint32_t x = (flags & 1) ? 0 : 5, y = (flags & 2) ? 0 : 6, z = (flags & 4) ? 0 : 7;
		if (face_flags(x, y, z) != flags) { printf("face_flags %u\n", flags); return 1; }
		const uint32_t owned = owned_slots(flags);
		for (uint32_t e = 0; e < 12; e++) {  // the clamped owner rule against owner_of on real coordinates
			const uint32_t ca = corner_code(edge_a(e));
			const OwnerRef o = owner_of(edge_axis(e), x + (ca & 1), y + ((ca >> 1) & 1), z + (ca >> 2));
			const uint32_t fo = face_owner(e, flags), self = o.x == x && o.y == y && o.z == z;
			if (self != (((owned >> e) & 1u) != 0) || self != ((fo & 15u) == 15u)) { printf("owner of edge %u flags %u\n", e, flags); return 2; }
			if (self) continue;
			static const int odx[6] = {1, 1, 1, 0, 0, 0}, ody[6] = {0, 0, 1, 0, 1, 1}, odz[6] = {1, 0, 0, 1, 0, 1};
			const uint32_t k = fo & 15u;
			if (k > 5 || x - o.x != (uint32_t)odx[k] || y - o.y != (uint32_t)ody[k] || z - o.z != (uint32_t)odz[k] || (fo >> 4) != o.e) {
				printf("face_owner edge %u flags %u\n", e, flags);
				return 3;
			}
		}
		for (uint32_t i = 1; i < 255; i++)
			for (uint32_t r = 0; r < per; r++) {
				float vb[8];
				Corner8 c8;
				for (int k = 0; k < 8; k++) {
					const uint32_t q = rnd();
					const float mag = (q & 7u) == 0 ? 1.0f : (float)((q >> 8) % 1000u + 1u) * ((q & 8u) ? 0.001f : 1.0f);
					vb[k] = ((i >> (7 - k)) & 1) ? -mag : mag;
					c8.a[k] = vb[k];
				}
				CellPlan p;
				plan_cell(p, tab, P, G, x, y, z, i, VRef{vb, 1});
				Entry want = make_entry(37, i, p, p.ntri, 11, 13, false);
				want.w3 |= ENTRY_TESTED | (flags ? ENTRY_FACE : 0u);
				uint32_t m, n;
				const uint32_t poff = pattern_offset(mc33_lut, i, c8, m, n);
				if (poff != p.poff) { printf("pattern i %u\n", i); return 4; }
				Entry got = make_face_entry(37, i, poff, (info[poff] >> 16) & 15u, order[poff], owned, 11, 13);
				if (!flags) got.w3 &= ~ENTRY_FACE;  // (an interior cell: the ranks a TESTED record carries)
				if (got.w0 != want.w0 || got.w1 != want.w1 || got.w2 != want.w2 || got.w3 != want.w3) {
					printf("record i %u flags %u: got %08x %08x %08x %08x want %08x %08x %08x %08x\n", i, flags, got.w0, got.w1, got.w2, got.w3, want.w0,
					       want.w1, want.w2, want.w3);
					return 5;
				}
				const Entry back = entry_join(entry_a(got), entry_b(got));
				if (back.w0 != got.w0 || back.w1 != got.w1 || back.w2 != got.w2 || back.w3 != got.w3) { printf("split i %u\n", i); return 6; }
				checked++;
			}
	}
	printf("ok %ld\n", checked);
	return 0;
}
