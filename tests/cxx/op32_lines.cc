// solver::use_fp32_operator_lines of the C++ mirror (include/cedar/multilevel.h), driven by tests/test_cxx_op32_lines.py:
// a 2D five-point solver on gallery::poisson with line-xy relaxation and the cycle of config.json switches the operator
// and line factors of its levels to single precision -- first with the default min_rows, then every level the call
// serves -- and runs pcg; the counts and the history are printed as one JSON line.
#include <cstdio>
#include <cedar/2d/solver.h>

using namespace cedar;

int main(int argc, char ** argv)
{
	const std::string out = argc > 1 ? argv[1] : ".";
	auto conf = std::make_shared<config>(out + "/config.json");
	log::status.on = false;
	const len_t nx = 141, ny = 129;
	auto so = cdr2::gallery::poisson(nx, ny);
	cdr2::grid_func b(nx, ny), x(nx, ny);
	for (len_t j = 1; j <= ny; j++)
		for (len_t i = 1; i <= nx; i++) b(i, j) = 1.0 / (1.0 + i + 2.0 * j);
	cdr2::solver<cdr2::five_pt> s(so, conf);
	const int point_call = s.use_fp32_operator_2d(1);
	const int by_default = s.use_fp32_operator_lines();
	const int every = s.use_fp32_operator_lines(1);
	s.pcg(b, x);
	std::printf("{\"nlevels\": %d, \"default\": %d, \"all\": %d, \"fp32_levels\": %d, \"point_call\": %d, \"h\": [", (int)s.nlevels(),
	            by_default, every, s.fp32_levels(), point_call);
	for (std::size_t i = 0; i < s.history.size(); i++) std::printf("%s%.17g", i ? ", " : "", s.history[i]);
	std::printf("]}\n");
	return 0;
}
