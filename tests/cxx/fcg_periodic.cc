// solver::fcg_periodic of the C++ mirror (include/cedar/multilevel.h), driven by tests/test_cxx_fcg_periodic.py on the
// periodic example configurations: the examples' periodic Poisson operator (five-point in 2D, seven-point in 3D, built
// as examples/ser-periodic-{2d,3d}.cc build it) with a rational right-hand side (no libm call, so that the Python side
// forms the same bits), the ghost layers of b filled with garbage.  pcg() and fcg() refuse the periodic solver;
// fcg_periodic() runs with the library's default pcg.* settings.  The history, samples of x and whether x came back
// with the periodic image in its ghosts are printed as one JSON line.
//   fcg_periodic <configuration file>
#include <array>
#include <cstdio>
#include <cedar/2d/solver.h>
#include <cedar/3d/solver.h>

using namespace cedar;

static cdr2::stencil_op<cdr2::five_pt> create_op2(len_t nx, len_t ny, std::array<bool, 3> periodic)
{
	using namespace cedar::cdr2;
	stencil_op<five_pt> so(nx, ny);
	so.set(0);
	const len_t mx = nx - (periodic[0] ? 1 : 0), my = ny - (periodic[1] ? 1 : 0);
	const real_t hx = 1.0 / (mx + 1), hy = 1.0 / (my + 1), xh = hy / hx, yh = hx / hy;
	const len_t l = so.shape(0), m = so.shape(1);
	const len_t ibeg = periodic[0] ? 1 : 2, jbeg = periodic[1] ? 1 : 2;
	for (len_t j = jbeg; j <= m; j++) for (len_t i = 1; i <= l; i++) so(i, j, five_pt::s) = 1.0 * yh;
	for (len_t j = 1; j <= m; j++) for (len_t i = ibeg; i <= l; i++) so(i, j, five_pt::w) = 1.0 * xh;
	for (auto j : so.range(1)) for (auto i : so.range(0)) so(i, j, five_pt::c) = 2 * xh + 2 * yh;
	const five_pt dirs[3] = { five_pt::c, five_pt::w, five_pt::s };
	if (periodic[0])
		for (auto j : so.range(1))
			for (auto d : dirs) {
				so(ibeg - 1, j, d) = so(l, j, d);
				so(l + 1, j, d) = so(ibeg, j, d);
			}
	if (periodic[1])
		for (auto i : so.range(0))
			for (auto d : dirs) {
				so(i, jbeg - 1, d) = so(i, m, d);
				so(i, m + 1, d) = so(i, jbeg, d);
			}
	return so;
}

static cdr3::stencil_op<cdr3::seven_pt> create_op3(len_t nx, len_t ny, len_t nz, std::array<bool, 3> per)
{
	using namespace cedar::cdr3;
	stencil_op<seven_pt> so(nx, ny, nz);
	so.set(0);
	const len_t mx = nx - (per[0] ? 1 : 0), my = ny - (per[1] ? 1 : 0), mz = nz - (per[2] ? 1 : 0);
	const real_t hx = 1.0 / (mx + 1), hy = 1.0 / (my + 1), hz = 1.0 / (mz + 1);
	const real_t xh = hy * hz / hx, yh = hx * hz / hy, zh = hx * hy / hz;
	const len_t l = so.shape(0), m = so.shape(1), n = so.shape(2);
	const len_t ibeg = per[0] ? 1 : 2, jbeg = per[1] ? 1 : 2, kbeg = per[2] ? 1 : 2;
	for (len_t k = 1; k <= n; k++) for (len_t j = jbeg; j <= m; j++) for (len_t i = 1; i <= l; i++) so(i, j, k, seven_pt::ps) = 1.0 * yh;
	for (len_t k = 1; k <= n; k++) for (len_t j = 1; j <= m; j++) for (len_t i = ibeg; i <= l; i++) so(i, j, k, seven_pt::pw) = 1.0 * xh;
	for (len_t k = kbeg; k <= n; k++) for (len_t j = 1; j <= m; j++) for (len_t i = 1; i <= l; i++) so(i, j, k, seven_pt::b) = 1.0 * zh;
	for (auto k : so.range(2)) for (auto j : so.range(1)) for (auto i : so.range(0)) so(i, j, k, seven_pt::p) = 2.0 * xh + 2.0 * yh + 2.0 * zh;
	const seven_pt dirs[4] = { seven_pt::p, seven_pt::pw, seven_pt::ps, seven_pt::b };
	if (per[0])
		for (auto k : so.grange(2)) for (auto j : so.grange(1)) for (auto d : dirs) {
			so(ibeg - 1, j, k, d) = so(l, j, k, d);
			so(l + 1, j, k, d) = so(ibeg, j, k, d);
		}
	if (per[1])
		for (auto k : so.grange(2)) for (auto i : so.grange(0)) for (auto d : dirs) {
			so(i, jbeg - 1, k, d) = so(i, m, k, d);
			so(i, m + 1, k, d) = so(i, jbeg, k, d);
		}
	if (per[2])
		for (auto j : so.grange(1)) for (auto i : so.grange(0)) for (auto d : dirs) {
			so(i, j, kbeg - 1, d) = so(i, j, n, d);
			so(i, j, n + 1, d) = so(i, j, kbeg, d);
		}
	return so;
}

// what the three calls left: pcg and fcg refused (empty history), fcg_periodic's history, x along the first interior row
// and whether the ghosts of x in the periodic directions equal the opposite interior end
template <class S, class G> static void report(S & s, const G & b, G & x, std::size_t row, std::size_t nrow)
{
	G xp(x), xf(x);
	s.pcg(b, xp);
	const std::size_t pcg_len = s.history.size();
	s.fcg(b, xf);
	const std::size_t fcg_len = s.history.size();
	s.fcg_periodic(b, x);
	std::printf("{\"pcg_len\": %zu, \"fcg_len\": %zu, \"hist\": [", pcg_len, fcg_len);
	for (std::size_t i = 0; i < s.history.size(); i++) std::printf("%s%.17g", i ? ", " : "", s.history[i]);
	std::printf("], \"x\": [");
	for (std::size_t i = 0; i < nrow; i++) std::printf("%s%.17g", i ? ", " : "", x.data()[row + i]);
	std::printf("]");
}

int main(int argc, char ** argv)
{
	if (argc < 2) return 2;
	auto conf = std::make_shared<config>(argv[1]);
	log::status.on = false;
	auto params = build_kernel_params(*conf);
	const auto per = params->periodic;
	auto n = conf->getvec<len_t>("grid.n");
	if (n.size() == 2) {
		const len_t nx = n[0], ny = n[1];
		auto so = create_op2(nx, ny, per);
		cdr2::grid_func b(nx, ny), x(nx, ny);
		b.set(-7.5); // garbage in the ghost layers of b: they must not matter
		x.set(0);
		for (len_t j = 1; j <= ny; j++)
			for (len_t i = 1; i <= nx; i++) b(i, j) = 1.0 / (1.0 + i + 2.0 * j);
		cdr2::solver<cdr2::five_pt> s(so, conf);
		const std::size_t II = nx + 2;
		report(s, b, x, II, II);
		bool ok = true;
		for (len_t j = 1; j <= ny && per[0]; j++) ok = ok && x(0, j) == x(nx, j) && x(nx + 1, j) == x(1, j);
		for (len_t i = 1; i <= nx && per[1]; i++) ok = ok && x(i, 0) == x(i, ny) && x(i, ny + 1) == x(i, 1);
		std::printf(", \"ghosts_ok\": %d}\n", (int)ok);
	} else {
		const len_t nx = n[0], ny = n[1], nz = n[2];
		auto so = create_op3(nx, ny, nz, per);
		cdr3::grid_func b(nx, ny, nz), x(nx, ny, nz);
		b.set(-7.5);
		x.set(0);
		for (len_t k = 1; k <= nz; k++)
			for (len_t j = 1; j <= ny; j++)
				for (len_t i = 1; i <= nx; i++) b(i, j, k) = 1.0 / (1.0 + i + 2.0 * j + 3.0 * k);
		cdr3::solver<cdr3::seven_pt> s(so, conf);
		const std::size_t II = nx + 2, JJ = ny + 2;
		report(s, b, x, II * JJ + II, II);
		bool ok = true;
		for (len_t k = 1; k <= nz; k++)
			for (len_t j = 1; j <= ny && per[0]; j++) ok = ok && x(0, j, k) == x(nx, j, k) && x(nx + 1, j, k) == x(1, j, k);
		for (len_t k = 1; k <= nz; k++)
			for (len_t i = 1; i <= nx && per[1]; i++) ok = ok && x(i, 0, k) == x(i, ny, k) && x(i, ny + 1, k) == x(i, 1, k);
		for (len_t j = 1; j <= ny; j++)
			for (len_t i = 1; i <= nx && per[2]; i++) ok = ok && x(i, j, 0) == x(i, j, nz) && x(i, j, nz + 1) == x(i, j, 1);
		std::printf(", \"ghosts_ok\": %d}\n", (int)ok);
	}
	return 0;
}
